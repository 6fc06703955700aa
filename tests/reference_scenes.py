"""The edge scenes on which the oracle and the HIP kernels are held to the reference's own kernels
(tests/test_gpu_reference_edges.py), and the conditions under which that comparison means something
(tests/test_reference_scenes_cpu.py).  Every scene is an existing generator at its committed size; nothing here calls the GPU.

  structured/*   tests/structured.py: all eight scenes at temperature 1; grid and iszero at 0.5; grid at 0
  tiequeue/*     tests/tie_queue_scenes.py: direct, tail, threshold, windows, none
  replay/*       tests/backward_replay_scenes.py: stack24, stack70 and opaque on both frames, temperatures 1 and 0
  camera/*       the three soups of tests/test_gpu_general_cameras.py under their general cameras, every view rendered
  desync/*       tests/desync_scene.py with K = 20 and K = 0

``SCENES[name]`` -> Scene(family, temp, build, present): ``build()`` the 21 boundary arguments (CPU tensors), ``present(args,
ref)`` asserts from the arguments and the oracle's forward ``ref`` that the scene still reaches the branch it exists for.
"""
import collections
import functools

import numpy as np

import backward_replay_scenes as brs
import cameras
import camera_grad_ref as cgr
import desync_scene
import structured as S
import tie_queue_scenes as TQ
from util import capture_forward_args, scenes

Scene = collections.namedtuple("Scene", "family temp build present")
SCENES = {}


# ---- structured ----------------------------------------------------------------------------------------------------------------
def _tie_count(args):
    b, f, pm = S.bbox_pairs(args)
    return int(S.exact_ties(args[12].numpy()[b, f], pm).sum()), len(b)


def _present_structured(name, temp):
    def check(args, ref):
        assert ref.num_rendered > 0 and (ref.final_T < 1).any()
        ties, pairs = _tie_count(args)
        assert ties >= 500, (ties, pairs)                                       # pairs on a pixel line or through a pixel corner
        if temp > 0:
            assert ref.buf_tri_cnt.max() > 0
        vi = args[9].numpy()
        if name in ("grid", "projected"):
            assert int(args[14].numpy().sum()) >= 6000                          # axis-parallel edges in the tables
        if name == "subpixel":
            v = args[12].numpy()
            assert (np.abs(v - np.round(v * 4) / 4) == 0).all() and (v.max(2) - v.min(2)).max() <= 4.0
        if name == "iszero":
            e = np.abs(args[13].numpy()).reshape(-1)
            assert (e == 0).sum() >= 100 and ((e > 0) & (e < 1e-3)).sum() >= 200 and ((e >= 1e-3) & (e < 1.6e-3)).sum() >= 100
        if name == "large":
            assert vi.shape[0] == 2 and (vi[..., 0] >= 3690).all() and (vi[..., 1] >= 1990).all()
            assert (args[1].numpy() >= [3700, 2000]).all()
        if name == "degenerate":
            v = args[12].numpy()
            a2 = (v[..., 1, 0] - v[..., 0, 0]) * (v[..., 2, 1] - v[..., 0, 1]) - (v[..., 2, 0] - v[..., 0, 0]) * (v[..., 1, 1] - v[..., 0, 1])
            assert (a2 == 0).sum() >= 300
        if name == "coplanar":
            fc = args[5].numpy()
            F = fc.shape[0] // 3
            assert np.array_equal(fc[:F], fc[F:2 * F]) and np.array_equal(fc[:F][:, [0, 2, 1]], fc[2 * F:])
        if name == "far":
            W, H = args[2], args[3]
            out = np.maximum(np.maximum(-vi[0, :, 0], vi[0, :, 0] - W), np.maximum(-vi[0, :, 1], vi[0, :, 1] - H))
            assert (out > 1e5).sum() >= 150 and (out > 5e6).sum() >= 60
    return check


for _name in S.ALL:
    _temps = {"grid": (1.0, 0.5, 0.0), "iszero": (1.0, 0.5)}.get(_name, (1.0,))
    for _t in _temps:
        SCENES[f"structured/{_name}_t{_t:g}".replace("0.5", "05")] = Scene(
            "structured", _t, functools.partial(S.make_args, _name, _t, 20), _present_structured(_name, _t))


# ---- the tie queue's scenes ----------------------------------------------------------------------------------------------------
def _present_ties(name):
    def check(args, ref):
        assert ref.num_rendered > 0 and ref.buf_tri_cnt.max() > 0
        ties, pairs = _tie_count(args)
        if name == "none":
            assert ties == 0, ties
        else:
            assert ties >= {"tail": 3, "windows": 2000}.get(name, 200), (ties, pairs)
        if name == "windows":
            assert args[9].shape[0] == 2 and (args[1].numpy()[1] != 0).all()
    return check


for _name in ("direct", "tail", "threshold", "windows", "none"):
    SCENES[f"tiequeue/{_name}"] = Scene("tiequeue", 1.0, functools.partial(TQ.make_args, _name), _present_ties(_name))


# ---- the backward replay's scenes ----------------------------------------------------------------------------------------------
REPLAY_N = (24, 70)                                  # the stacks of tests/test_gpu_backward_replay.py


def _replay(kind, frame, temp):
    return brs.opaque_scene(frame, temp) if kind == "opaque" else brs.stack_scene(frame, int(kind[5:]), temp)


def _present_replay(kind, frame, temp):
    def check(args, ref):
        info = _replay(kind, frame, temp)[1]
        if kind == "opaque":
            brs.present_guard(args, ref, info)                                  # (present_opaque is its first step)
        else:
            brs.present_stack(args, ref, info)
            if info["n"] > 30:
                assert (ref.n_contrib > 30).any()
    return check


for _kind in [f"stack{n}" for n in REPLAY_N] + ["opaque"]:
    for _frame in brs.FRAMES:
        for _t in (1.0, 0.0):
            SCENES[f"replay/{_kind}_{_frame}_t{_t:g}"] = Scene(
                "replay", _t, (lambda k=_kind, f=_frame, t=_t: _replay(k, f, t)[0]), _present_replay(_kind, _frame, _t))


# ---- general cameras -----------------------------------------------------------------------------------------------------------
CAM_W, CAM_H, CAM_F = 96, 72, 600                    # W, H, F of tests/test_gpu_general_cameras.py
CAM_SEED = scenes.SEED_BASE + 5


@functools.lru_cache(maxsize=None)
def camera_scene(name):
    return {
        "soup": lambda: cameras.reposed_soup(CAM_W, CAM_H, CAM_F, CAM_SEED, 3, shared_verts=True),
        "grazing": lambda: cameras.grazing_soup(CAM_W, CAM_H, CAM_F, CAM_SEED, 2, shared_verts=True),
        "dense": lambda: cameras.reposed_soup(CAM_W, CAM_H, CAM_F, CAM_SEED + 10, 2, mix=cameras.MIX_DENSE, shared_verts=True),
    }[name]()


@functools.lru_cache(maxsize=None)
def _camera_args(name):
    sc = camera_scene(name)
    B = sc.mv.shape[0]
    return tuple(capture_forward_args(sc, list(range(B)), [[0, 0]] * B, CAM_W, CAM_H, 1.0, 20)[0])


def _present_camera(name):
    def check(args, ref):
        sc = camera_scene(name)
        assert (sc.mv[:, :3, :4] != 0).all()                                    # three-axis rotations: no exact zero
        assert np.abs(sc.mv[0, :3, :3].numpy() - sc.mv[0, :3, :3].numpy().T).max() > 0.1
        assert ref.num_rendered > 0 and (ref.final_T[: CAM_W * CAM_H] < 1).mean() > 0.5
        av, vi, fc = args[12].numpy(), args[9].numpy(), args[5].numpy()
        flipped = np.any(av[:, :, 1] != vi[:, fc[:, 1]], axis=-1)
        assert flipped.any(axis=1).all() and (~flipped).any(axis=1).all()        # both windings in every view
        if name == "dense":
            assert (sc.proj[:, 2, :2] != 0).all()                               # x and y mixed into clip z
        if name == "grazing":
            pos, neg = cgr.clamp_masks(sc.verts, sc.mv, sc.proj)
            assert pos[-1].sum() >= 8 and neg[-1].sum() >= 8 and np.abs(vi).max() > 1e5      # vertices inside the |w| clamp
    return check


for _name in ("soup", "grazing", "dense"):
    SCENES[f"camera/{_name}"] = Scene("camera", 1.0, (lambda n=_name: list(_camera_args(n))), _present_camera(_name))


# ---- the desync corner ---------------------------------------------------------------------------------------------------------
def _present_desync(K):
    def check(args, ref):
        v = args[4].numpy().reshape(-1, 3, 3)
        deg = np.arange(desync_scene.F) % desync_scene.EVERY == 0
        assert (v[deg, 0] == v[deg, 1]).all() and not (v[~deg, 0] == v[~deg, 1]).all(-1).any()
        cnt = ref.buf_tri_cnt
        if K == 0:
            assert cnt.max() == 0 and ref.buf_tri_id.size == 0
            return
        # a degenerate face's record on top of a pixel's stack, behind the pixel's last contributor, blended faces under it
        top = np.take_along_axis(ref.buf_tri_id, np.maximum(cnt - 1, 0)[..., None], axis=-1)[..., 0]
        stuck = (cnt >= 2) & (cnt < K) & deg[top] & (ref.n_contrib.reshape(cnt.shape) > 0)
        assert stuck.sum() >= 20, int(stuck.sum())
    return check


for _K in (20, 0):
    SCENES[f"desync/k{_K}"] = Scene("desync", 1.0, functools.partial(desync_scene.desync_args, _K), _present_desync(_K))

FAMILIES = ("structured", "tiequeue", "replay", "camera", "desync")


@functools.lru_cache(maxsize=None)
def args(name):
    """The scene's 21 arguments, built once (read-only)."""
    return tuple(SCENES[name].build())


def names(family=None):
    return [n for n, s in SCENES.items() if family is None or s.family == family]


def centres_on_edges(a):
    """(B, H, W) bool: the pixels whose centre lies exactly on an edge (end points included) of one of the scene's faces in
    image space -- where a ray meets its face with u, v or 1 - u - v equal to 0 up to rounding.  fp64 on fp32 inputs of
    lattice size: the differences and products are exact, the zero test is too."""
    v = a[12].numpy().astype(np.float64)                                        # (B,F,3,2)
    pm = a[1].numpy().astype(np.float64)
    W, H = int(a[2]), int(a[3])
    out = np.zeros((v.shape[0], H, W), dtype=bool)
    ys, xs = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    for b in range(v.shape[0]):
        cx, cy = (xs + pm[b, 0]).reshape(-1, 1), (ys + pm[b, 1]).reshape(-1, 1)  # (N,1)
        hit = np.zeros(H * W, dtype=bool)
        for i in range(3):
            p, q = v[b, :, i], v[b, :, (i + 1) % 3]                              # (F,2)
            cross = (q[:, 0] - p[:, 0]) * (cy - p[:, 1]) - (q[:, 1] - p[:, 1]) * (cx - p[:, 0])
            inside = (np.minimum(p[:, 0], q[:, 0]) <= cx) & (cx <= np.maximum(p[:, 0], q[:, 0])) \
                & (np.minimum(p[:, 1], q[:, 1]) <= cy) & (cy <= np.maximum(p[:, 1], q[:, 1]))
            hit |= ((cross == 0) & inside).any(axis=1)
        out[b] = hit.reshape(H, W)
    return out
