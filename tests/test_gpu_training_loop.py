"""The op as a training loop drives it: one Renderer called again and again with one shape and changing geometry (the
binning-buffer hint of ``_C.render_forward_cuda`` and both call sequences through the C ABI behind it), several forwards before
their backwards, a caller on a side stream while the GPU is busy, and callers on several threads.

Every comparison is against the references and bars the suite already has: the CPU oracle bit-exact in the forward and within
GRAD_TOL relative L-inf in the gradients (util.check_forward / check_backward / check_from_image), the fused prep against the
oracle's at its own 1e-6 (test_gpu_prep.py), the layered ops against their restatements (layer_composite_ref, rasterize_ref,
interpolate_ref, texture_ref).  The scenes of one shape come from tests/sequence.py (held to their conditions on the CPU by
tests/test_sequence_cpu.py).  Which call sequence a step took is read from a spy on the C entry points, never assumed: a step
that does not take the route it was built for fails with a message saying so."""
import contextlib
import threading

import numpy as np
import pytest
import torch

import interpolate_ref as iref
import layer_composite_ref as lref
import rasterize_ref as rref
import sequence as seq
import texture_ref as tref
from util import (GRAD_NAMES, GRAD_TOL, check_backward, check_forward, check_from_image, from_image_oracle_args, patched_C,
                  pool_state, rel_linf, run_both, scatter_aa_grad_to_verts, scenes, spy_library, to_dev, to_numpy_args)

import dmesh2_renderer_amd as dm2
from dmesh2_renderer_amd import _C

pytestmark = pytest.mark.gpu

B, W, H, F = len(seq.VIEWS), seq.W, seq.H, seq.F
PREP_TOL = 1e-6         # the fused prep's backward against the oracle's (test_gpu_prep.py)
PLAN_THEN_RUN = [("dm2_forward", 2), ("dm2_forward_run", 0)]
ONE_CALL = [("dm2_forward", 0)]


def _orc():
    from oracle import cpu as orc
    return orc


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _key():
    return (torch.cuda.current_device(), B, W, H, F)


def _binning_bytes(R):
    return _C.load_library().dm2_scratch_bytes(_C.SCRATCH_BINNING, R, _C._tiles(B, W, H))


def _pool_bytes(pairs):
    return _C.load_library().dm2_scratch_bytes(_C.SCRATCH_PAIR_POOL, pairs, 0)


def _upstream(shape_bhw, seed):
    rng = np.random.RandomState(seed)
    return rng.randn(*shape_bhw, 3).astype(np.float32), rng.randn(*shape_bhw).astype(np.float32)


# ---- the spy on the C entry points ------------------------------------------------------------------------------------------
@contextlib.contextmanager
def library_calls():
    """-> a list that receives one dict per call of dm2_forward / dm2_forward_run (fn, rc, the bytes of binning scratch
    handed over, the forward mode reported; for the plan-and-run call also R and the pair bound) and of dm2_backward (fn, R,
    the forward mode told)."""
    lib = _C.load_library()
    log = []

    def fwd(name, bin_at):
        real = getattr(lib, name)

        def f(*a):
            rc = real(*a)
            e = dict(fn=name, rc=rc, bin_bytes=int(a[bin_at]), mode=int(a[-1]._obj.value))
            if bin_at == 4:
                e.update(R=int(a[-4]._obj.value), pairs=int(a[-2]._obj.value))
            log.append(e)
            return rc
        return f

    def bwd(name):
        real = getattr(lib, name)

        def f(*a):
            log.append(dict(fn="dm2_backward", R=int(a[1]), mode=int(a[2])))
            return real(*a)
        return f

    with spy_library(dm2_forward=fwd("dm2_forward", 4), dm2_forward_run=fwd("dm2_forward_run", 7), dm2_backward=bwd("dm2_backward")):
        yield log


def _forwards(log):
    return [(e["fn"], e["rc"]) for e in log if e["fn"].startswith("dm2_forward")]


@contextlib.contextmanager
def recorded_backwards():
    """-> a list of (num_rendered, the six gradients) of every _C.render_backward_cuda (autograd's thread included)."""
    seen = []
    real = _C.render_backward_cuda

    def rec(*a, **kw):
        g = real(*a, **kw)
        seen.append((int(a[0]), g))
        return g

    with patched_C(render_backward_cuda=rec):
        yield seen


# ---- B1. one shape, changing scene ------------------------------------------------------------------------------------------
class Arena:
    """Stands in for ``_C._bytes``: the scratch buffers of a forward (face, image, binning, in the order render_forward_cuda asks
    for them) and the backward's tie queue come from tensors that live across the steps, grown when too small (the old contents
    carried over) and never cleared: each step works in the memory the previous step left behind, contents intact."""

    def __init__(self):
        self.slots, self.phase, self.n = {}, "fwd", 0

    def begin(self, phase):
        self.phase, self.n = phase, 0

    def bytes(self, dev, n):
        n = max(int(n), 0)
        if self.phase == "fwd":
            # the slots go by the order of the forward's requests; held to the sizes of the face and image scratch of this shape and
            # to at most two requests for binning scratch (the hint's, the re-run's), so that a request added to the shim later
            # fails here instead of being served live scratch
            lib, Tn = _C.load_library(), _C._tiles(B, W, H)
            want = (lib.dm2_scratch_bytes(_C.SCRATCH_FACE, B * F, 2 * Tn + 1), lib.dm2_scratch_bytes(_C.SCRATCH_IMAGE, B * H * W, Tn))
            assert self.n < 4, f"request {self.n + 1} for scratch in one forward: the arena knows face, image, binning, binning"
            assert self.n >= 2 or n == want[self.n], f"forward request {self.n} asks for {n} B, expected {want[self.n]} B"
            name = ("face", "image", "binning", "binning")[self.n]
        else:
            assert self.n == 0, "the backward asks for one scratch buffer, its tie queue"
            name = "tie"
        self.n += 1
        buf = self.slots.get(name)
        if buf is None or buf.numel() < n:
            new = torch.zeros((n + n // 2 + 256,), dtype=torch.uint8, device=dev)
            if buf is not None:
                new[:buf.numel()] = buf
            buf = self.slots[name] = new
        return buf[:n]

    @contextlib.contextmanager
    def installed(self):
        real_f, real_b = _C.render_forward_cuda, _C.render_backward_cuda

        def f(*a):
            self.begin("fwd")
            return real_f(*a)

        def b(*a, **kw):
            self.begin("bwd")
            return real_b(*a, **kw)

        with patched_C(_bytes=self.bytes, render_forward_cuda=f, render_backward_cuda=b):
            yield self


def _op_step(args, seed, from_image):
    """One forward + backward of the op on the 21 CPU arguments against the oracle, at the suite's bars."""
    if from_image:
        gc, gd = _upstream((B, int(args[3]), int(args[2])), seed)
        return check_from_image(to_dev(args), torch.from_numpy(gc).cuda(), torch.from_numpy(gd).cuda(), tol=GRAD_TOL)
    res = run_both(args, seed=seed)
    check_forward(res, args)
    return check_backward(res)


def _check_route(name, log, before, wants_pool=True):
    """The forward calls of one step against the hint it met: one call when the buffer of ``before`` bytes holds what the plan
    asked for, plan-allocate-run otherwise.  -> the plan's log entry."""
    fw = [e for e in log if e["fn"].startswith("dm2_forward")]
    assert fw and fw[0]["fn"] == "dm2_forward", (name, log)
    first = fw[0]
    assert first["bin_bytes"] == before, f"{name}: the forward was handed {first['bin_bytes']} B of binning scratch, the hint was {before}"
    need = _binning_bytes(first["R"]) + (_pool_bytes(first["pairs"]) if wants_pool else 0)
    want = ONE_CALL if need <= before else PLAN_THEN_RUN
    assert _forwards(log) == want, f"{name}: need {need} B, hint {before} B, calls {_forwards(log)}"
    return first, need


@pytest.mark.parametrize("scratch", ["allocator", "arena"])
@pytest.mark.parametrize("from_image", [False, True], ids=["tables", "from_image"])
def test_one_shape_changing_scene(from_image, scratch):
    """S0..S6 under one hint key, nothing freed in between: every step against the oracle, and the call sequence each step took."""
    _C._bin_hint.clear()
    with contextlib.ExitStack() as es:
        log = es.enter_context(library_calls())
        if scratch == "arena":
            es.enter_context(Arena().installed())
        seen = es.enter_context(recorded_backwards())
        keep = []                                                  # (the steps' gradients stay alive; no cache is emptied)
        for k, name in enumerate(seq.ORDER):
            del log[:], seen[:]
            before = _C._bin_hint.get(_key(), 0)
            worst = _op_step(seq.step_args(name), 100 + k, from_image)
            after = _C._bin_hint.get(_key(), 0)
            first, need = _check_route(name, log, before)
            route = _forwards(log)
            print(name, "R", first["R"], "pairs", first["pairs"], "hint", before, "->", after, route, worst)
            keep.append(seen[:])
            if name != "S5":
                assert first["R"] > 0 and _C.last_forward_mode() == _C.FWD_POOL, (name, _C.last_forward_mode())
                assert all(e["mode"] == _C.FWD_POOL for e in log if e["fn"] == "dm2_backward"), (name, log)
            if name == "S0":
                assert before == 0 and route == PLAN_THEN_RUN, f"S0 must start without a buffer: hint {before}, {route}"
            elif name in ("S1", "S3"):
                assert route == ONE_CALL, f"{name} was built to fit the buffer of the step before: need {need}, hint {before}"
            elif name == "S2":
                assert before > 0 and route == PLAN_THEN_RUN, f"S2 was built to outgrow S1's buffer: need {need}, hint {before}"
            elif name == "S4":
                assert route == ONE_CALL and after < before, f"S4 was built to fit and to shrink the hint: {before} -> {after}, {route}"
            elif name == "S5":
                assert first["R"] == 0 and route == ONE_CALL, (first, route)
                assert seen and all(not x.any() for _, g in seen for x in g), "S5 renders nothing: every gradient is exactly zero"
                assert after < before, f"the empty step was to shrink the hint: {before} -> {after}"
            # (S6: whichever the hint the empty step left dictates -- _check_route holds it to that)


@pytest.mark.parametrize("scratch", ["allocator", "arena"])
@pytest.mark.parametrize("from_image", [False, True], ids=["tables", "from_image"])
def test_binning_fits_pool_missing(from_image, scratch):
    """T0 (temperature 0: no pair pool) leaves a hint of 1.25 x the binning part; T1 (same scene, temperature 1) fits its binning
    part in that buffer and misses only the pool: dm2_forward is handed the buffer, returns 2, and the re-run keeps a pool.  With
    the arena the re-run (tile ranges not cleared by the plan) works in the grown buffer that still holds T0's note of its mode,
    keys and lists at the very offsets T1 uses (same num_rendered)."""
    _C._bin_hint.clear()
    with contextlib.ExitStack() as es:
        log = es.enter_context(library_calls())
        if scratch == "arena":
            es.enter_context(Arena().installed())
        _op_step(seq.step_args("S0", 0.0), 201, from_image)
        R = log[0]["R"]
        nb = _binning_bytes(R)
        assert _forwards(log) == PLAN_THEN_RUN and _C.last_forward_mode() == _C.FWD_POINT
        assert _C._bin_hint[_key()] == nb + nb // 4, "T0 must leave a hint for the binning part alone"
        del log[:]
        _op_step(seq.step_args("S0", 1.0), 202, from_image)
        first = log[0]
        assert first["R"] == R
        assert _C.last_pair_bound() > 4 * R, f"the pool must not fit the 25 % slack: {_C.last_pair_bound()} pairs, R {R}"
        assert first["bin_bytes"] >= nb, f"T1 was to be handed a buffer that holds its binning part: {first['bin_bytes']} < {nb}"
        assert _forwards(log) == PLAN_THEN_RUN, f"T1 was built to miss only the pool: {_forwards(log)}"
        assert _C.last_forward_mode() == _C.FWD_POOL
        assert all(e["mode"] == _C.FWD_POOL for e in log if e["fn"] == "dm2_backward")


# ---- the module against the oracle ------------------------------------------------------------------------------------------
class ModuleRun:
    """One Renderer.forward on a scene (device tensors; fused prep, tables from the image: the product default) whose backward
    may come later.  ``verify`` holds the forward to the oracle bit for bit on the very arguments the op got, the op's six
    gradients to the oracle's within GRAD_TOL, the leaves verts_color / faces_opacity / faces_intense likewise, and verts.grad to
    the op's own gradients taken through the oracle's prep backward within the prep's 1e-6."""

    def __init__(self, r, sc, seed, temp=1.0, views=seq.VIEWS, pm=None, pw=None, ph=None, **fwd_kw):
        self.r, self.sc, self.temp, self.views, self.fwd_kw = r, sc, temp, list(views), fwd_kw
        self.pw, self.ph = pw or r.width, ph or r.height
        self.pm = pm or [[0, 0]] * len(self.views)
        g = torch.Generator().manual_seed(seed)
        n = len(self.views)
        self.wc_host = torch.randn((n, self.ph, self.pw, 3), generator=g)
        self.wd_host = torch.randn((n, self.ph, self.pw), generator=g)
        self.leaves = [x.detach().clone().requires_grad_(True)
                       for x in (sc.verts, sc.verts_color, sc.faces_opacity, sc.faces_intense[self.views])]

    def forward(self, weights=None, mid=None):
        """-> the loss <wc, color> + <wd, depth>; ``mid`` runs between the op's forward and the loss (``weights``: its device
        tensors, when they are to arrive late)."""
        got = {}
        real = _C.render_forward_cuda

        def spy(*a):
            got["args"] = a
            return real(*a)

        pm = torch.tensor(self.pm, dtype=torch.int64, device="cuda")
        with patched_C(render_forward_cuda=spy):
            self.out = self.r(self.views, pm, self.pw, self.ph, self.leaves[0], self.sc.faces, self.leaves[1], self.leaves[2],
                              self.leaves[3], self.sc.background, aa_temperature=self.temp, **self.fwd_kw)
        self.mode = _C.last_forward_mode()
        self.args = got["args"]
        assert self.args[12].shape[1] == 0, "the default Renderer hands the op placeholders for the AA tables"
        if mid is not None:
            mid()
        wc, wd = weights if weights is not None else (self.wc_host.cuda(), self.wd_host.cuda())
        self.loss = (self.out[0] * wc).sum() + (self.out[1] * wd).sum()
        return self.loss

    def oracle(self):
        orc = _orc()
        self.na = from_image_oracle_args([a.detach() if torch.is_tensor(a) else a for a in self.args])
        self.ref = orc.render_forward_cuda(*self.na)
        # Renderer's depth is 1 - (z + 1) / 2 of the op's: the op got -wd / 2
        self.gref = orc.render_backward_cuda(self.ref, self.wc_host.numpy(), (self.wd_host * -0.5).numpy())
        return self.ref

    def verify_forward(self):
        ref = self.oracle()
        c, d = self.out[0].detach().cpu().numpy(), self.out[1].detach().cpu().numpy()
        assert np.array_equal(_bits(c), _bits(ref.color)), f"colour max abs diff {np.abs(c - ref.color).max()}"
        want_d = np.float32(1.0) - (ref.depth + np.float32(1.0)) / np.float32(2.0)
        assert np.array_equal(_bits(d), _bits(want_d)), f"depth max abs diff {np.abs(d - want_d).max()}"
        return ref

    def verify(self, op_grads):
        """``op_grads``: the six gradients _C.render_backward_cuda returned for this forward (the sixth routed to the vertices)."""
        ref, gref, na = self.verify_forward(), self.gref, self.na
        g = [x.detach().cpu().numpy() for x in op_grads]
        worst = {}
        for name, x in zip(GRAD_NAMES[:5], g):
            assert x.shape == gref[name].shape, name
            worst[name] = rel_linf(x, gref[name])
        worst["aa_to_verts"] = rel_linf(g[5], scatter_aa_grad_to_verts(gref["aa_face_verts"], na[12], na[9], na[5]))
        leaf = [x.grad.cpu().numpy() for x in self.leaves]
        for i, name in ((1, "verts_color"), (2, "faces_opacity"), (3, "faces_intense")):
            worst["leaf_" + name] = rel_linf(leaf[i], gref[name])
        assert all(v <= GRAD_TOL for v in worst.values()), worst
        if ref.num_rendered > 0:
            assert np.abs(gref["verts_color"]).max() > 0 and np.abs(gref["faces_opacity"]).max() > 0
        # verts.grad = the op's dL/dverts + the prep's backward of the op's dL/dverts_ndc and dL/dverts_image
        sc = self.sc
        mv, proj = sc.mv[self.views].cpu().numpy(), sc.proj[self.views].cpu().numpy()
        through = _orc().prepare_faces_backward(sc.verts.cpu().numpy(), sc.faces.cpu().numpy(), mv, proj, self.r.width, self.r.height,
                                                g_ndc=g[3], g_image=g[5])
        # (the prep's own bar, test_gpu_prep.py: relative L-inf against the reference; autograd's fp32 sum of the two terms adds
        # half an ulp, 6e-8)
        want = g[0].astype(np.float64) + through
        worst["leaf_verts"] = rel_linf(leaf[0], want)
        assert worst["leaf_verts"] <= PREP_TOL, f"verts.grad differs from the op's gradients through the prep: {worst['leaf_verts']}"
        return worst


def _module_loop(names, **kw):
    """Renderer.forward + loss.backward() over the named steps with ONE Renderer -> per step (ModuleRun, the calls' log)."""
    sc0 = seq.scene(names[0]).to("cuda")
    r = dm2.Renderer(sc0.mv, sc0.proj, W, H, "cuda")
    done = []
    with library_calls() as log, recorded_backwards() as seen:
        for k, name in enumerate(names):
            del log[:], seen[:]
            before = _C._bin_hint.get(_key(), 0)
            run = ModuleRun(r, seq.scene(name).to("cuda"), 300 + k, **kw)
            run.forward().backward()
            torch.cuda.synchronize()
            assert len(seen) == 1
            worst = run.verify(seen[0][1])
            _check_route(name, log, before)
            print(name, _forwards(log), worst)
            done.append((run, list(log), before))
    return done


def test_module_training_loop():
    """Renderer(...)(...) + loss.backward() over S0, S2, S4, S0 with one Renderer: grow, shrink, and the first scene again."""
    _C._bin_hint.clear()
    done = _module_loop(["S0", "S2", "S4", "S0"])
    routes = [_forwards(log) for _, log, _ in done]
    assert routes[0] == PLAN_THEN_RUN and routes[1] == PLAN_THEN_RUN and routes[2] == ONE_CALL, routes
    assert done[3][2] < done[2][2], "S4 was to shrink the hint"
    for run, log, _ in done:
        assert [e["mode"] for e in log if e["fn"] == "dm2_backward"] == [run.mode] == [_C.FWD_POOL]


def _oracle_weights(na):
    """The face weights of the float32 oracle: dL/dfaces_intense of the unit-colour scene for dL/dcolor = (1, 0, 0)
    (test_gpu_face_weights.py)."""
    orc = _orc()
    na = list(na)
    na[6] = np.ones_like(na[6])
    ref = orc.render_forward_cuda(*na)
    gc = np.zeros(ref.color.shape, np.float32); gc[..., 0] = 1.0
    return orc.render_backward_cuda(ref, gc, np.zeros(ref.depth.shape, np.float32))["faces_intense"]


def test_module_alpha_and_weights_over_budget_with_a_stale_larger_buffer():
    """return_alpha + return_face_weights over S0, S2, S0; on the last step the pair pool is over budget although S2's larger
    buffer is at hand and has room for it: dm2_forward composites with a pool, the shim renders again with masks only
    (dm2_forward_run), and the weights are those of ONE composite."""
    _C._bin_hint.clear()
    sc0 = seq.scene("S0").to("cuda")
    r = dm2.Renderer(sc0.mv, sc0.proj, W, H, "cuda")
    with library_calls() as log, recorded_backwards() as seen:
        for k, name in enumerate(["S0", "S2", "S0"]):
            del log[:], seen[:]
            last = k == 2
            run = ModuleRun(r, seq.scene(name).to("cuda"), 320 + k, return_alpha=True, return_face_weights=True)
            with patched_C(_pool_budget=(lambda N, R: 1) if last else _C._pool_budget):
                run.forward().backward()
            torch.cuda.synchronize()
            assert len(run.out) == 4 and len(seen) == 1
            run.verify(seen[0][1])
            alpha, fw = run.out[2].detach().cpu().numpy(), run.out[3].cpu().numpy()
            want_a = np.float32(1.0) - run.ref.final_T.reshape(alpha.shape)
            assert np.array_equal(_bits(alpha), _bits(want_a))
            want_w = _oracle_weights(run.na)
            assert np.array_equal(fw > 0, want_w != 0) and (fw > 0).sum() >= 10
            assert rel_linf(fw, want_w) <= GRAD_TOL, rel_linf(fw, want_w)
            told = [e["mode"] for e in log if e["fn"] == "dm2_backward"]
            if last:
                fwd = [(e["fn"], e["rc"], e["mode"]) for e in log if e["fn"].startswith("dm2_forward")]
                assert fwd == [("dm2_forward", 0, _C.FWD_POOL), ("dm2_forward_run", 0, _C.FWD_MASKS)], \
                    f"the last step was to composite with a pool in S2's buffer and render again with masks only: {fwd}"
                assert run.mode == _C.FWD_MASKS and told == [_C.FWD_MASKS]
            else:
                assert run.mode == _C.FWD_POOL and told == [_C.FWD_POOL]


# ---- B2. forwards before backwards ------------------------------------------------------------------------------------------
def _bwd(out, dargs, gc, gd):
    return _C.render_backward_cuda(out[0], *dargs, gc, gd, out[7], out[8], out[9], out[3], out[4], out[5], out[6])


def test_three_forwards_then_their_backwards():
    """Under one key: S0 at temperature 1 (keeps a pair pool), S2 at temperature 0 (point coverage), S3 with no pool budget
    (blend masks only); then the backwards in the order S0, S3, S2, each against the oracle and each told the mode of ITS
    forward (from the note on the binning buffer it is handed)."""
    orc = _orc()
    _C._bin_hint.clear()
    plan = [("S0", 1.0, None, _C.FWD_POOL), ("S2", 0.0, None, _C.FWD_POINT), ("S3", 1.0, 0, _C.FWD_MASKS)]
    runs = {}
    with library_calls() as log:
        for name, temp, bud, want_mode in plan:
            args = seq.step_args(name, temp)
            dargs = to_dev(args)
            with patched_C(_pool_budget=_C._pool_budget if bud is None else (lambda N, R: bud)):
                out = _C.render_forward_cuda(*dargs)
            assert _C.last_forward_mode() == want_mode, f"{name} was to leave mode {want_mode}, left {_C.last_forward_mode()}"
            runs[name] = dict(args=args, dargs=dargs, out=out, pool=pool_state(out), mode=want_mode)
        for k, name in enumerate(["S0", "S3", "S2"]):
            run = runs[name]
            ref = run["ref"] = orc.render_forward_cuda(*to_numpy_args(run["args"]))
            gc, gd = _upstream(ref.depth.shape, 400 + k)
            del log[:]
            grads = _bwd(run["out"], run["dargs"], torch.from_numpy(gc).cuda(), torch.from_numpy(gd).cuda())
            run["grads"] = [g.cpu().numpy() for g in grads]
            run["ref_grads"] = orc.render_backward_cuda(ref, gc, gd)
            told = [(e["R"], e["mode"]) for e in log if e["fn"] == "dm2_backward"]
            assert told == [(ref.num_rendered, run["mode"])], f"{name}: the backward was told {told}, its forward left {run['mode']}"
        torch.cuda.synchronize()
    for name, run in runs.items():
        check_forward(run, run["args"])
        print(name, check_backward(run))


def test_module_three_losses_one_backward():
    """The same through the module: three Renderer.forward calls that leave different modes, the losses summed, one backward();
    every RenderFunction.backward tells the kernel the mode of its own forward (held on ctx with the forward's side channels)."""
    _C._bin_hint.clear()
    sc0 = seq.scene("S0").to("cuda")
    r = dm2.Renderer(sc0.mv, sc0.proj, W, H, "cuda")
    plan = [("S0", 1.0, None, _C.FWD_POOL), ("S2", 0.0, None, _C.FWD_POINT), ("S3", 1.0, 0, _C.FWD_MASKS)]
    runs, loss = [], 0.0
    with library_calls() as log, recorded_backwards() as seen:
        for k, (name, temp, bud, want_mode) in enumerate(plan):
            run = ModuleRun(r, seq.scene(name).to("cuda"), 410 + k, temp=temp)
            with patched_C(_pool_budget=_C._pool_budget if bud is None else (lambda N, R: bud)):
                loss = loss + run.forward()
            assert run.mode == want_mode, f"{name} was to leave mode {want_mode}, left {run.mode}"
            runs.append(run)
        loss.backward()
        torch.cuda.synchronize()
        told = {e["R"]: e["mode"] for e in log if e["fn"] == "dm2_backward"}
        by_R = {R: g for R, g in seen}
        assert len(seen) == 3 and len(by_R) == 3
        for run in runs:
            R = run.oracle().num_rendered
            assert told.get(R) == run.mode, f"the backward of the forward with R = {R} was told {told.get(R)}, its forward left {run.mode}"
            print(R, run.verify(by_R[R]))


def test_patchwise_gradients_accumulate_to_the_full_frame():
    """One frame rendered as two patches (rows of batch_patch_min, patch_height = H / 2) in two forwards, the losses summed: the
    patches are the oracle's full frame bit for bit, and the op's accumulated gradients its full-frame gradients."""
    orc = _orc()
    _C._bin_hint.clear()
    sc = seq.scene("S2").to("cuda")
    r = dm2.Renderer(sc.mv, sc.proj, W, H, "cuda")
    ph = H // 2
    leaves = None
    runs, loss = [], 0.0
    with recorded_backwards() as seen:
        for k in range(2):
            run = ModuleRun(r, sc, 420 + k, views=[0], pm=[[0, k * ph]], ph=ph)
            if leaves is None:
                leaves = run.leaves
            run.leaves = leaves                                    # (both patches render the same leaves)
            loss = loss + run.forward()
            runs.append(run)
        loss.backward()
        torch.cuda.synchronize()
    assert len(seen) == 2
    na = from_image_oracle_args([a.detach() if torch.is_tensor(a) else a for a in runs[0].args])
    na[1] = np.zeros((1, 2), np.int32)
    na[3] = H
    na[19], na[20] = r.ray_o[0:1].cpu().numpy(), r.ray_d[0:1].cpu().numpy()
    ref = orc.render_forward_cuda(*na)
    for k, run in enumerate(runs):
        c, d = run.out[0].detach().cpu().numpy(), run.out[1].detach().cpu().numpy()
        rows = slice(k * ph, (k + 1) * ph)
        assert np.array_equal(_bits(c), _bits(np.ascontiguousarray(ref.color[:, rows])))
        want_d = np.float32(1.0) - (ref.depth[:, rows] + np.float32(1.0)) / np.float32(2.0)
        assert np.array_equal(_bits(d), _bits(np.ascontiguousarray(want_d)))
    gc = np.concatenate([run.wc_host.numpy() for run in runs], axis=1)
    gd = np.concatenate([(run.wd_host * -0.5).numpy() for run in runs], axis=1)
    gref = orc.render_backward_cuda(ref, gc, gd)
    total = [sum(g[i].double() for _, g in seen).cpu().numpy() for i in range(6)]
    worst = {name: rel_linf(x, gref[name]) for name, x in zip(GRAD_NAMES[:5], total)}
    worst["aa_to_verts"] = rel_linf(total[5], scatter_aa_grad_to_verts(gref["aa_face_verts"], na[12], na[9], na[5]))
    for i, name in ((1, "verts_color"), (2, "faces_opacity"), (3, "faces_intense")):
        worst["leaf_" + name] = rel_linf(leaves[i].grad.cpu().numpy(), gref[name])
    print(worst)
    assert np.abs(gref["verts"]).max() > 0
    assert all(v <= GRAD_TOL for v in worst.values()), worst


# ---- B3. a side stream with the GPU kept busy ----------------------------------------------------------------------------------
_RATE = {}


def _cycles_per_ms():
    if "r" not in _RATE:
        torch.cuda._sleep(1_000_000)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); torch.cuda._sleep(4_000_000); e1.record()
        e1.synchronize()
        _RATE["r"] = 4_000_000 / max(e0.elapsed_time(e1), 1e-3)
    return _RATE["r"]


class Delay:
    """About 30 ms of spinning enqueued on ``stream``; ``check`` asserts from events that it really took 10 ms or more (a delay,
    not a measurement: nothing is judged by it, but without it the test would prove nothing)."""

    def __init__(self, stream, ms=30.0):
        cycles = int(ms * _cycles_per_ms())
        self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            self.e0.record(); torch.cuda._sleep(cycles); self.e1.record()

    def check(self):
        self.e1.synchronize()
        t = self.e0.elapsed_time(self.e1)
        assert t >= 10.0, f"the delay took {t} ms: the GPU was not kept busy and the test proves nothing"


def _busy(which, side):
    """The delay in front of the op's work: on the op's own stream ('side': everything the op enqueues there runs behind it, and
    anything it enqueues elsewhere runs before its inputs arrive), or on the default stream with the op's stream free."""
    return Delay(side if which == "side" else torch.cuda.default_stream())


_LANES = []


def _sides():
    """Two side streams, made one after the other and kept for the whole module; every stream case runs on both.  An
    assumption about the runtime, not something this project controls: streams are spread over a few hardware queues (four by
    default), handed out in turn, and a stream that shares its queue with the null stream runs in order with it -- there a
    launch that went to the null stream by mistake waits behind the side stream's delay like everything else and nothing shows.
    Under that assumption at most one of two streams made in a row shares the null stream's queue.

    The two ``busy`` variants are not redundant either.  With the delay on the side stream, the forward's read-back of the plan
    makes the host wait the delay out, so only the launches up to that read-back (and those behind the second delay, up to the
    first host wait) are certainly ahead of their inputs.  With the default stream busy instead, anything that went there by
    mistake has not run when the results are read, however many host waits the op has."""
    if not _LANES:
        _LANES.extend([torch.cuda.Stream(), torch.cuda.Stream()])
    return _LANES


class Staged:
    """Device tensors born on the default stream holding poison that is itself a valid, different scene; the real values wait in
    pinned host memory for ``upload`` (an asynchronous copy on the current stream)."""

    def __init__(self, real, poison):
        self.host = [x.detach().contiguous().pin_memory() for x in real]
        self.dev = [p.detach().to(x.dtype).contiguous().cuda() for x, p in zip(real, poison)]

    def upload(self):
        with torch.no_grad():
            for d, h in zip(self.dev, self.host):
                d.copy_(h, non_blocking=True)


def _zeros(xs):
    return [torch.zeros_like(x) for x in xs]


def _staged_args(args):
    """The 21 arguments on the device, poisoned: every tensor zero (faces all vertex 0, no colour, no rays) but verts_ndc, which
    is the real one moved behind the far plane -- an empty, culled scene: well defined and in bounds, but wrong."""
    idx = [i for i, a in enumerate(args) if torch.is_tensor(a)]
    real = [args[i] for i in idx]
    poison = _zeros(real)
    poison[idx.index(8)] = args[8] + 10.0
    st = Staged(real, poison)
    dargs = list(args)
    for i, d in zip(idx, st.dev):
        dargs[i] = d
    return st, dargs


@pytest.mark.parametrize("busy", ["side", "default"])
@pytest.mark.parametrize("from_image", [False, True], ids=["tables", "from_image"])
@pytest.mark.parametrize("temp", [1.0, 0.0])
def test_side_stream_op(temp, from_image, busy):
    """_C.render_forward_cuda / render_backward_cuda on a side stream: the inputs arrive on that stream behind a delay (or with
    the default stream kept busy instead), the upstream gradients behind a second one; nothing but the side stream is waited for."""
    for side in _sides():
        _side_stream_op(temp, from_image, busy, side)


def _side_stream_op(temp, from_image, busy, side):
    orc = _orc()
    args = seq.step_args("S0", temp)
    na = from_image_oracle_args(args) if from_image else to_numpy_args(args)
    ref = orc.render_forward_cuda(*na)
    gc, gd = _upstream(ref.depth.shape, 500)
    gref = orc.render_backward_cuda(ref, gc, gd)
    st, dargs = _staged_args(args)
    if from_image:
        for k in range(12, 18):
            dargs[k] = dargs[k][:, :0]                              # placeholders: the plan builds the tables from verts_image
    ups = Staged([torch.from_numpy(gc), torch.from_numpy(gd)], [torch.zeros(gc.shape), torch.zeros(gd.shape)])
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        d1 = _busy(busy, side)
        st.upload()
        with _C.tables_from_image(from_image), _C.aa_grad_to_verts(from_image):
            out = _C.render_forward_cuda(*dargs)
        mode = _C.last_forward_mode()
        d2 = _busy(busy, side)
        ups.upload()
        with _C.tables_from_image(from_image):
            grads = _bwd(out, dargs, *ups.dev)
            routed = None
            if from_image:
                with _C.aa_grad_to_verts(True):
                    routed = _bwd(out, dargs, *ups.dev)[5]
        side.synchronize()
        # (the results are read before anything waits for the delays: with the default stream busy, work that went there by
        # mistake has not run yet)
        res = dict(out=out, ref=ref, grads=[g.cpu().numpy() for g in grads], ref_grads=gref)
        assert mode == (_C.FWD_POOL if temp > 0 else _C.FWD_POINT)
        check_forward(res, args)
        worst = check_backward(res)
        if from_image:
            worst["aa_to_verts"] = rel_linf(routed.cpu().numpy(), scatter_aa_grad_to_verts(gref["aa_face_verts"], na[12], na[9], na[5]))
            assert worst["aa_to_verts"] <= GRAD_TOL, worst
        assert np.abs(gref["verts"]).max() > 0
        print(worst)
        d1.check(); d2.check()
    torch.cuda.synchronize()


def _far(verts):
    v = verts.clone()
    v[:, 2] -= seq.FAR_SHIFT
    return v


@pytest.mark.parametrize("busy", ["side", "default"])
def test_side_stream_module(busy):
    """Renderer.forward + loss.backward() inside the stream context: autograd's thread follows the forward's stream."""
    for side in _sides():
        _side_stream_module(busy, side)


def _side_stream_module(busy, side):
    _C._bin_hint.clear()
    sc = seq.scene("S1")
    real = [sc.verts, sc.faces, sc.verts_color, sc.faces_opacity, sc.faces_intense]
    st = Staged(real, [_far(sc.verts)] + _zeros(real[1:]))
    scd = sc.to("cuda")
    scd.verts, scd.faces, scd.verts_color, scd.faces_opacity, scd.faces_intense = st.dev
    r = dm2.Renderer(scd.mv, scd.proj, W, H, "cuda")
    run = ModuleRun(r, scd, 510)
    lv = Staged([sc.verts, sc.verts_color, sc.faces_opacity, sc.faces_intense[seq.VIEWS]],
                [_far(sc.verts), torch.zeros_like(sc.verts_color), torch.zeros_like(sc.faces_opacity), torch.zeros_like(sc.faces_intense)])
    run.leaves = [x.requires_grad_(True) for x in lv.dev]
    ups = Staged([run.wc_host, run.wd_host], _zeros([run.wc_host, run.wd_host]))
    torch.cuda.synchronize()
    with torch.cuda.stream(side), recorded_backwards() as seen:
        d1 = _busy(busy, side)
        st.upload(); lv.upload()
        delays = []

        def mid():                                                 # (a second delay in front of the loss and the backward)
            delays.append(_busy(busy, side))
            ups.upload()

        run.forward(weights=ups.dev, mid=mid).backward()
        side.synchronize()
        assert len(seen) == 1 and run.mode == _C.FWD_POOL
        run.sc = sc.to("cuda")                                     # (the real scene, for the prep's reference)
        print(run.verify(seen[0][1]))
        d1.check(); delays[0].check()
    torch.cuda.synchronize()


@pytest.mark.parametrize("busy", ["side", "default"])
def test_side_stream_prepare_faces(busy):
    """prepare_faces / prepare_faces_backward alone: forward bit-equal to the oracle's, backward within its 1e-6."""
    for side in _sides():
        _side_stream_prepare_faces(busy, side)


def _side_stream_prepare_faces(busy, side):
    orc = _orc()
    sc = seq.scene("S0")
    keys = ("verts_ndc", "verts_image", "verts", "edges", "iszero", "recip", "normal", "normal_c")
    ref = orc.prepare_faces(sc.verts, sc.faces, sc.mv, sc.proj, W, H)
    P = sc.verts.shape[0]
    gen = torch.Generator().manual_seed(520)
    ups_real = [torch.randn((B, P, 3), generator=gen), torch.randn((B, P, 2), generator=gen), torch.randn((B, F, 3, 2), generator=gen)]
    gref = orc.prepare_faces_backward(sc.verts, sc.faces, sc.mv, sc.proj, W, H, *ups_real)
    st = Staged([sc.verts, sc.faces], [_far(sc.verts), torch.zeros_like(sc.faces)])
    ups = Staged(ups_real, _zeros(ups_real))
    mv, proj = sc.mv.cuda(), sc.proj.cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        d1 = _busy(busy, side)
        st.upload(); ups.upload()
        outs = _C.prepare_faces(st.dev[0], st.dev[1], mv, proj, W, H)
        g = _C.prepare_faces_backward(st.dev[0], st.dev[1], mv, proj, W, H, *ups.dev)
        side.synchronize()
        got = [o.cpu().numpy() for o in outs] + [g.cpu().numpy()]  # (read before anything waits for the delay)
        for k, o in zip(keys, got):
            assert np.array_equal(_bits(o), _bits(ref[k])), k
        assert rel_linf(got[-1], gref) <= PREP_TOL
        d1.check()
    torch.cuda.synchronize()


def _layered_check(busy, side):
    """LayeredRenderer.generate against the oracle (exact), then LayeredRenderer.render of those layers + loss.backward()
    against layer_composite_ref on the very arguments the compositor got: forward bit-equal, the op's four gradients and the
    leaves within GRAD_TOL."""
    orc = _orc()
    Wl, Hl, L, bidx = 96, 80, 4, [0, 1]
    ts = scenes.tet_lattice(Wl, Hl, 4, seed=scenes.SEED_BASE + 930, num_cams=2)
    names = ("verts", "faces", "tets", "face_tets", "tet_faces", "faces_existence")
    real = [getattr(ts, n) for n in names]
    st = Staged(real, [_far(ts.verts)] + _zeros(real[1:]))
    P, Fl = ts.verts.shape[0], ts.faces.shape[0]
    rng = np.random.RandomState(7)
    mat_real = [torch.from_numpy(rng.uniform(0, 1, (P, 3)).astype(np.float32)), torch.from_numpy(rng.uniform(0.05, 0.95, Fl).astype(np.float32)),
                torch.from_numpy(rng.uniform(0.5, 1.5, (2, Fl)).astype(np.float32))]
    mat = Staged(mat_real, _zeros(mat_real))
    for x in mat.dev:
        x.requires_grad_(True)
    gen = torch.Generator().manual_seed(530)
    ups_real = [torch.randn((2, Hl, Wl, 3), generator=gen), torch.randn((2, Hl, Wl), generator=gen)]
    ups = Staged(ups_real, _zeros(ups_real))
    lr = dm2.LayeredRenderer(ts.mv.cuda(), ts.proj.cuda(), Wl, Hl, "cuda")
    bgd = torch.tensor([0.1, 0.3, 0.7]).cuda()
    torch.cuda.synchronize()
    got = {}
    real_gen, real_comp, real_cb = _C.generate_render_layers_cuda, _C.composite_layers_cuda, _C.composite_layers_backward_cuda

    def spy_gen(*a):
        got["gen"] = a
        return real_gen(*a)

    def spy_comp(*a):
        got["comp"] = a
        return real_comp(*a)

    def spy_cb(*a, **kw):
        got["grads"] = real_cb(*a, **kw)
        return got["grads"]

    with torch.cuda.stream(side), patched_C(generate_render_layers_cuda=spy_gen, composite_layers_cuda=spy_comp,
                                            composite_layers_backward_cuda=spy_cb):
        d1 = _busy(busy, side)
        st.upload(); mat.upload()
        layers, cnt = lr.generate(bidx, *st.dev, L)
        color, depth = lr.render(bidx, layers, st.dev[0], st.dev[1], mat.dev[0], mat.dev[1], mat.dev[2], bgd)
        d2 = _busy(busy, side)
        ups.upload()
        ((color * ups.dev[0]).sum() + (depth * ups.dev[1]).sum()).backward()
        side.synchronize()
        op_grads = [x.cpu().numpy() for x in got["grads"]]         # (read before anything waits for the delays)
        leaf = [x.grad.cpu().numpy() for x in mat.dev]
        la = [a.detach().cpu().numpy() if torch.is_tensor(a) else a for a in got["gen"]]
        rl, rc = orc.generate_render_layers_cuda(*la)
        assert np.array_equal(layers.cpu().numpy(), rl) and np.array_equal(cnt.cpu().numpy(), rc), "layers differ from the oracle's"
        assert int(rc.sum()) > 1000
        cargs = [a.detach().cpu() for a in got["comp"]]
        fwd = lref.forward32(*cargs)
        assert fwd["blend"].sum() > 1000
        assert np.array_equal(_bits(color.detach().cpu().numpy()), _bits(fwd["color"]))
        want_d = np.float32(1.0) - (fwd["depth_raw"] + np.float32(1.0)) / np.float32(2.0)
        assert np.array_equal(_bits(depth.detach().cpu().numpy()), _bits(want_d))
        # Renderer's depth is 1 - (z + 1) / 2 of the op's: the op got -wd / 2
        want = lref.grads64(fwd, *cargs[2:8], ups_real[0].double(), (ups_real[1] * -0.5).double())
        for name, x in zip(("verts_color", "faces_opacity", "verts_ndc", "faces_intense"), op_grads):
            assert rel_linf(x, want[name]) <= GRAD_TOL, (name, rel_linf(x, want[name]))
        for name, x in zip(("verts_color", "faces_opacity", "faces_intense"), leaf):
            assert np.abs(want[name]).max() > 0 and rel_linf(x, want[name]) <= GRAD_TOL, ("leaf " + name, rel_linf(x, want[name]))
        d1.check(); d2.check()
    torch.cuda.synchronize()


@pytest.mark.parametrize("busy", ["side", "default"])
def test_side_stream_layered(busy):
    """LayeredRenderer.generate and .render + loss.backward() on a side stream."""
    for side in _sides():
        _layered_check(busy, side)


def _chain_inputs(seed):
    Wc, Hc = 80, 64
    sc = scenes.triangle_soup(Wc, Hc, 600, scenes.SEED_BASE + seed, num_cams=2, depth_complexity=12.0, shared_verts=True)
    gen = torch.Generator().manual_seed(seed)
    Fc = sc.faces.shape[0]
    uv_faces = torch.arange(3 * Fc, dtype=torch.int32).reshape(Fc, 3)
    table = torch.rand((3 * Fc, 2), generator=gen) * 2 - 0.5
    tex = torch.randn((64, 64, 3), generator=gen)
    wgt = torch.randn((2, Hc, Wc, 4, 3), generator=gen)
    return sc, uv_faces, table, tex, wgt


def _chain_run(r, bidx, verts, faces, table, uv_faces, tex, wgt, mid=None):
    """rasterize -> interpolate -> texture -> a weighted sum, backward (test_gpu_texture.py's module path)."""
    layers, cnt, bary, t = r.rasterize(bidx, verts, faces, 4)
    uv = r.interpolate(layers, bary, table, uv_faces)
    out = r.texture(uv, tex, layers, boundary_mode="wrap")
    if mid is not None:
        mid()
    (out * wgt).sum().backward()
    return layers, cnt, bary, uv, out


def _chain_verify(r, bidx, res, real, grads):
    """``real``: (verts, faces, table, uv_faces, tex, wgt) as CPU tensors; ``grads``: (verts.grad, table.grad, tex.grad)."""
    layers, cnt, bary, uv, out = res
    verts0, faces, table0, uv_faces, tex0, wgt = real
    ro, rd = r._camera_rows(r.ray_o, bidx).cpu().numpy(), r._camera_rows(r.ray_d, bidx).cpu().numpy()
    assert int(cnt.sum()) > 3000
    rl, bn, un, gn = (x.detach().cpu().numpy() for x in (layers, bary, uv, wgt))
    tn = tex0.numpy()
    assert np.array_equal(_bits(un), _bits(iref.forward32(rl, bn, table0.numpy(), uv_faces.numpy())))
    assert np.array_equal(_bits(out.detach().cpu().numpy()), _bits(tref.forward32(un, tn, rl, "linear", "wrap")))
    wt, wu = tref.grads64(un, tn, rl, "linear", "wrap", gn)
    wtab, wb = iref.grads64(rl, bn, table0.numpy(), uv_faces.numpy(), wu)
    wv = rref.grads64(verts0.numpy(), faces.numpy(), rl, ro, rd, wb, None)
    gv, gtab, gt = (g.cpu().numpy() for g in grads)
    worst = dict(tex=rel_linf(gt, wt), table=rel_linf(gtab, wtab), verts=rel_linf(gv, wv))
    assert np.abs(wt).max() > 0 and np.abs(wtab).max() > 0 and np.abs(wv).max() > 0
    assert all(v <= GRAD_TOL for v in worst.values()), worst
    return worst


@pytest.mark.parametrize("busy", ["side", "default"])
def test_side_stream_rasterize_interpolate_texture(busy):
    """rasterize -> interpolate -> texture with gradients to verts, the UV table and the texture, on a side stream."""
    for side in _sides():
        _side_stream_chain(busy, side)


def _side_stream_chain(busy, side):
    sc, uv_faces, table, tex, wgt = _chain_inputs(940)
    bidx = [1, 0]
    st = Staged([sc.verts, sc.faces, table, uv_faces, tex], [_far(sc.verts), torch.zeros_like(sc.faces), torch.zeros_like(table),
                                                             torch.zeros_like(uv_faces), torch.zeros_like(tex)])
    ups = Staged([wgt], _zeros([wgt]))
    r = dm2.LayeredRenderer(sc.mv.cuda(), sc.proj.cuda(), sc.width, sc.height, "cuda")
    verts, faces, tab, uvf, tx = st.dev
    for x in (verts, tab, tx):
        x.requires_grad_(True)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        d1 = _busy(busy, side)
        st.upload()
        delays = []

        def mid():
            delays.append(_busy(busy, side))
            ups.upload()

        res = _chain_run(r, bidx, verts, faces, tab, uvf, tx, ups.dev[0], mid)
        side.synchronize()
        grads = [x.grad.cpu() for x in (verts, tab, tx)]           # (read before anything waits for the delays)
        res = [x.detach().cpu() for x in res]
        print(_chain_verify(r, bidx, res, (sc.verts, sc.faces, table, uv_faces, tex, wgt), grads))
        d1.check(); delays[0].check()
    torch.cuda.synchronize()


# ---- B4. threads ------------------------------------------------------------------------------------------------------------
def _run_threads(workers, timeout=240.0):
    """Start the workers together (a barrier), each on a stream of its own; collect what they raise and raise it here.  Every
    worker gets ``meet``: all workers wait there for each other (they call it the same number of times)."""
    barrier = threading.Barrier(len(workers))
    errors = []

    def body(i, fn):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                barrier.wait(timeout=60.0)
                fn(lambda: barrier.wait(timeout=120.0))
                torch.cuda.current_stream().synchronize()
        except BaseException as ex:                                # noqa: BLE001 (re-raised in the main thread)
            import traceback
            errors.append((i, fn.__name__, ex, traceback.format_exc()))
            barrier.abort()

    threads = [threading.Thread(target=body, args=(i, fn), name=f"dm2-test-{i}") for i, fn in enumerate(workers)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=timeout)
    torch.cuda.synchronize()
    alive = [t.name for t in threads if t.is_alive()]
    assert not alive, f"threads still running after {timeout} s: {alive}"
    if errors:
        # (a thread that failed breaks the barrier for the others: show the failure, not the broken barrier)
        errors.sort(key=lambda e: isinstance(e[2], threading.BrokenBarrierError))
        i, name, ex, tb = errors[0]
        raise AssertionError(f"{len(errors)} of {len(workers)} threads failed; thread {i} ({name}):\n{tb}") from ex


def _shifted_tables(args):
    """``args`` with AA tables of the caller's own (the corners shifted by (3.5, -2.25), the other five rebuilt from them without
    reordering, as test_gpu_parity.caller_tables does): a call that builds its tables from verts_image instead renders another
    image."""
    orc = _orc()
    a = list(args)
    v = np.ascontiguousarray(args[12].numpy() + np.array([3.5, -2.25], np.float32), dtype=np.float32)
    Bv, Fv = v.shape[:2]
    t = orc.aa_tables(v.reshape(-1, 3, 2), np.float32, reorder=False)
    for k, name in zip(range(12, 17), ("verts", "edges", "iszero", "recip", "normal")):
        a[k] = torch.from_numpy(np.ascontiguousarray(t[name].reshape(Bv, Fv, 3, 2)))
    a[17] = torch.from_numpy(np.ascontiguousarray(t["normal_c"].reshape(Bv, Fv, 3)))
    return a


def _soup_args(Ws, Hs, Fs, seed, dc, temp):
    from util import soup_args
    return soup_args(Ws, Hs, Fs, scenes.SEED_BASE + seed, temp=temp, cams=2, batch_idx=(0, 1), depth_complexity=dc)[0]


STEPS_PER_THREAD = 5


def test_four_threads_with_their_own_switches():
    """Four threads released together, each with its own stream, scene shape and per-thread switches, five forward + backward
    steps alternating two scenes: (a) caller-supplied AA tables, (b) tables_from_image + aa_grad_to_verts, (c) temperature 0
    with alpha_output, (d) rasterize -> interpolate -> texture.  Each thread sets its switches, all meet, every thread runs its
    forward and backward, all meet again, and only then the switches are taken back.  A switch that leaks from one thread into another changes what
    that one computes or returns."""
    orc = _orc()
    a_args = [_shifted_tables(_soup_args(112, 80, 700, 950, 4.0, 1.0)), _shifted_tables(_soup_args(112, 80, 700, 951, 12.0, 1.0))]
    b_args = [_soup_args(96, 96, 900, 952, 3.0, 1.0), _soup_args(96, 96, 900, 953, 20.0, 1.0)]
    c_args = [_soup_args(128, 64, 500, 954, 4.0, 0.0), _soup_args(128, 64, 500, 955, 15.0, 0.0)]
    d_in = [_chain_inputs(956), _chain_inputs(957)]
    d_r = dm2.LayeredRenderer(d_in[0][0].mv.cuda(), d_in[0][0].proj.cuda(), d_in[0][0].width, d_in[0][0].height, "cuda")
    torch.cuda.synchronize()

    # every step: each thread sets its switches, all meet, all work, all meet again, and only then the switches are taken back --
    # whatever a thread computes, it computes while the other threads' switches are set
    def tables(meet):
        for k in range(STEPS_PER_THREAD):
            args = a_args[k % 2]
            meet()
            try:
                res = run_both(args, seed=600 + k)
            finally:
                meet()
            assert len(res["out"]) == 10
            check_forward(res, args)
            check_backward(res)

    def from_image(meet):
        from dmesh2_renderer_amd.sharding import BandShardedOp
        for k in range(STEPS_PER_THREAD):
            args = b_args[k % 2]
            na = from_image_oracle_args(args)
            ref = orc.render_forward_cuda(*na)
            gc, gd = _upstream(ref.depth.shape, 610 + k)
            gref = orc.render_backward_cuda(ref, gc, gd)
            a = BandShardedOp(to_dev(args), 1, 0, tables_from_image=True).args
            with _C.tables_from_image(True), _C.aa_grad_to_verts(True):
                meet()
                try:
                    out = _C.render_forward_cuda(*a)
                    grads = [g.cpu().numpy() for g in _bwd(out, a, torch.from_numpy(gc).cuda(), torch.from_numpy(gd).cuda())]
                finally:
                    meet()
            assert len(out) == 10 and out[0] == ref.num_rendered
            for i, want in ((1, ref.color), (2, ref.depth), (5, ref.buf_tri_cnt)):
                assert np.array_equal(_bits(out[i].cpu().numpy()), _bits(want)), i
            worst = {name: rel_linf(x, gref[name]) for name, x in zip(GRAD_NAMES[:5], grads)}
            assert grads[5].shape == (2, a[4].shape[0], 2)
            worst["aa_to_verts"] = rel_linf(grads[5], scatter_aa_grad_to_verts(gref["aa_face_verts"], na[12], na[9], na[5]))
            assert all(v <= GRAD_TOL for v in worst.values()), worst

    def point_alpha(meet):
        for k in range(STEPS_PER_THREAD):
            args = c_args[k % 2]
            dargs = to_dev(args)
            ref = orc.render_forward_cuda(*to_numpy_args(args))
            gc, gd = _upstream(ref.depth.shape, 620 + k)
            with _C.alpha_output(True):
                meet()
                try:
                    out = _C.render_forward_cuda(*dargs)
                    mode = _C.last_forward_mode()
                    grads = _bwd(out, dargs, torch.from_numpy(gc).cuda(), torch.from_numpy(gd).cuda())
                finally:
                    meet()
            assert len(out) == 11 and mode == _C.FWD_POINT
            assert grads[5].shape == (2, 500, 3, 2)
            res = dict(out=out[:10], ref=ref, grads=[g.cpu().numpy() for g in grads], ref_grads=orc.render_backward_cuda(ref, gc, gd))
            check_forward(res, args)
            check_backward(res)
            alpha = out[10].cpu().numpy()
            assert np.array_equal(_bits(alpha), _bits(np.float32(1.0) - ref.final_T.reshape(alpha.shape)))

    def chain(meet):
        for k in range(STEPS_PER_THREAD):
            sc, uv_faces, table, tex, wgt = d_in[k % 2]
            verts, tab, tx = (x.cuda().requires_grad_(True) for x in (sc.verts, table, tex))
            meet()
            try:
                res = _chain_run(d_r, [1, 0], verts, sc.faces.cuda(), tab, uv_faces.cuda(), tx, wgt.cuda())
            finally:
                meet()
            _chain_verify(d_r, [1, 0], res, (sc.verts, sc.faces, table, uv_faces, tex, wgt), (verts.grad, tab.grad, tx.grad))

    _run_threads([tables, from_image, point_alpha, chain])


def test_two_threads_share_one_hint_key():
    """Two threads on the SAME (device, B, W, H, F): they share the binning-buffer hint, one alternating S0 / S2, the other
    S4 / S3, so each keeps meeting a hint the other left (too small, or far too large)."""
    _C._bin_hint.clear()

    def small_large(meet):
        for k in range(STEPS_PER_THREAD):
            _op_step(seq.step_args(("S0", "S2")[k % 2]), 700 + k, k % 2 == 1)

    def tiny_large(meet):
        for k in range(STEPS_PER_THREAD):
            _op_step(seq.step_args(("S4", "S3")[k % 2]), 710 + k, k % 2 == 0)

    _run_threads([small_large, tiny_large])
    assert list(_C._bin_hint) == [_key()]
