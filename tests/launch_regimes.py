"""The launch-time regimes of the per-slot ops and who tests them ("Launch regimes and who tests them").

Three things, none of which needs a GPU (tests/test_launch_regimes_cpu.py holds them to the sources):

``sweep``        a model of the forwards' sweep over a block's nslots * CV outputs, step for step as tex_sweep (dm2_tex_core.h) and its
                 three written-out copies form it, with three wrong variants;
``hash_levels``  check_hash_grid's resolutions and hg_levels' dense word, in integers;
``TABLE``        one row per (op, kernel, regime): the launcher's condition, quoted, and the test that enters it.

and the parameter lists of tests/test_gpu_launch_regimes.py, which the census reads from here.
"""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dmesh2_renderer_amd", "csrc")
BLOCK = 256                                      # TEX_BLOCK, IP_BLOCK: lanes of a flat block

# ---- the sweep ------------------------------------------------------------------------------------------------------------------
VARIANTS = ("carry omitted", "dq floored at 1", "> for >= in the carry")


def sweep(tid, nslots, CV, variant=None):
    """[(e, slot, group)] lane ``tid`` visits: e = tid, tid + 256, ... below nslots * CV; (slot, group) stepped by
    dq = 256 / CV, dr = 256 - dq * CV with a single carry.  ``variant``: one of VARIANTS, a wrong kernel."""
    assert variant is None or variant in VARIANTS
    total = nslots * CV
    dq = BLOCK // CV
    if variant == "dq floored at 1":
        dq = max(dq, 1)
    dr = BLOCK - dq * CV
    slot = tid // CV
    c = tid - slot * CV
    out = []
    for e in range(tid, total, BLOCK):
        out.append((e, slot, c))
        slot += dq
        c += dr
        if variant == "carry omitted":
            continue
        if (c > CV) if variant == "> for >= in the carry" else (c >= CV):
            c -= CV
            slot += 1
    return out


def sweep_is_right(nslots, CV, variant=None):
    return all((slot, c) == divmod(e, CV) for tid in range(BLOCK) for e, slot, c in sweep(tid, nslots, CV, variant))


def sweeps_wrong(nslots, CVs, variant=None):
    """``sweep`` for every lane and every CV of ``CVs`` at once (numpy, the same steps) -> bool per CV: some lane visits something
    other than divmod(e, CV)."""
    import numpy as np
    assert variant is None or variant in VARIANTS
    CV = np.asarray(CVs, np.int64)[:, None]
    tid = np.arange(BLOCK, dtype=np.int64)[None, :]
    total = nslots * CV
    dq = BLOCK // CV
    if variant == "dq floored at 1":
        dq = np.maximum(dq, 1)
    dr = BLOCK - dq * CV
    slot = tid // CV
    c = tid - slot * CV
    e = tid + 0 * CV
    wrong = np.zeros(CV.shape[0], bool)
    while (e < total).any():
        live = e < total
        wrong |= (live & ((slot != e // CV) | (c != e % CV))).any(1)
        slot = slot + dq
        c = c + dr
        if variant != "carry omitted":
            carry = (c > CV) if variant == "> for >= in the carry" else (c >= CV)
            c = np.where(carry, c - CV, c)
            slot = slot + carry
        e = e + BLOCK
    return wrong


REGIMES = ("dq >= 2, dr > 0", "dq >= 2, dr == 0", "dq == 1, dr > 0", "dq == 1, dr == 0", "dq == 0")


def sweep_regime(CV):
    dq = BLOCK // CV
    dr = BLOCK - dq * CV
    if dq == 0:
        return "dq == 0"
    return f"dq {'>= 2' if dq >= 2 else '== 1'}, dr {'> 0' if dr else '== 0'}"


# the four places the stepping is written: (file, kernel(s), block constant, the name of CV there)
SWEEPS = (("dm2_tex_core.h", "tex_sweep: k_texture, k_texture_cube, k_texture_volume", "TEX_BLOCK", "CV"),
          ("dm2_interpolate.hip", "k_interpolate", "IP_BLOCK", "C"),
          ("dm2_texture_mip.hip", "k_texture_mip", "TEX_BLOCK", "CV"),
          ("dm2_texture_cube.hip", "k_texture_cube_mip", "TEX_BLOCK", "CV"))
TEX_SWEEP_CALLERS = ("dm2_texture.hip", "dm2_texture_cube.hip", "dm2_texture_volume.hip")


def stepping_lines(block, cv):
    """The lines ``sweep`` restates, as the sources write them."""
    return (f"const int dq = {block} / {cv}, dr = {block} - dq * {cv};",
            f"int slot = tid / {cv}, c = tid - slot * {cv};",
            f"for (int e = tid; e < total; e += {block}) {{",
            "slot += dq; c += dr;",
            f"if (c >= {cv}) {{ c -= {cv}; slot++; }}")


# ---- the hash grid's levels -------------------------------------------------------------------------------------------------------
def hash_levels(N, growth16, NL, log2T):
    """(R[0 .. NL - 1], dense word) as check_hash_grid (dm2_api.hip) and hg_levels (dm2_hash_grid.hip) form them; ValueError where
    check_hash_grid refuses the levels."""
    if not (1 <= NL <= 32 and 17 <= growth16 <= 32 and 4 <= log2T <= 24 and N >= 1):
        raise ValueError("levels, growth, rows or base resolution out of range")
    R, r = [], N
    for _ in range(NL):
        if r > 1 << 20:
            raise ValueError("finest resolution above 2^20")
        R.append(r)
        r = (r * growth16) >> 4
    dense = 0
    for v in range(NL):
        if R[v] * R[v] * R[v] <= 1 << log2T:
            dense |= 1 << v
    return R, dense


# ---- the parameter lists of tests/test_gpu_launch_regimes.py --------------------------------------------------------------------
OLD_CS = tuple(range(1, 34))                     # every C the op files' lists could hold: they stop at 33 (cube, volume: 16)
SCALAR_CS = (131, 256, 259)                      # C % 4 != 0, or (256) tables 4 bytes into their storage: CV = C
VECTOR_CS = (12, 516, 1024, 1028)                # aligned, C % 4 == 0: CV = C / 4 = 3, 129, 256, 257
WIDE_SHAPES = ((1, 7, 37, 1), (2, 4, 5, 2))      # 259 slots: one full block and a ragged one of 3; two views, per-view tables
WIDE_OPS = ("interpolate", "texture", "texture_mip", "texture_cube", "texture_cube_mip", "texture_volume")


def wide_cases(op):
    """[(C, shifted)] of ``op``: interpolate's forward has no vector path (its C % 4 == 0 values run the vector path of the bary
    backward)."""
    return [(C, C % 4 == 0) for C in SCALAR_CS] + [(C, False) for C in VECTOR_CS]


def wide_cv(op, C, shifted):
    return C // 4 if (C % 4 == 0 and not shifted and op != "interpolate") else C


# name -> (N, growth16, NL, log2T, the Fs it runs at); the positions, shapes and modes are the test's
HASH_CASES = {
    "32 levels": (16, 17, 32, 12, (1, 2)),            # level 0 dense with R^3 == T, 31 hashed levels, R up to 70
    "32 levels, 17 dense": (16, 17, 32, 15, (2,)),    # R <= 32 dense: bits 0 .. 16 of the dense word
    "32 levels, all dense": (16, 17, 32, 19, (1,)),   # 70^3 <= 2^19: the dense word is 0xFFFFFFFF, bit 31 included
    "workload": (16, 24, 16, 19, (2,)),               # the layout the op was added for
    "finest 2^20": (1 << 20, 32, 1, 16, (2,)),
    "finest 2^19, 2^20": (1 << 19, 32, 2, 16, (2,)),
    "2^24 rows, dense": (256, 32, 1, 24, (1,)),       # R^3 == T: the table filled exactly
    "2^24 rows, hashed": (257, 32, 1, 24, (1,)),
}

MAX_VIEWS = 65535                                # a grid's y and z extents
MAX_ROWS = 16 * 65535                            # H whose tile rows are 65535
# op -> the shapes (B, H, W, L) at its bounds and one step past them; hash_grid's views are B * NL (NL: 15 at, 16 past)
SLOT_GRID_OPS = ("texture", "texture_mip", "texture_cube", "texture_cube_mip", "texture_volume", "interpolate")
AT_BOUND = ((MAX_VIEWS, 1, 1, 1), (1, MAX_ROWS, 1, 1))
PAST_BOUND = ((MAX_VIEWS + 1, 1, 1, 1), (1, MAX_ROWS + 1, 1, 1))
HASH_AT_BOUND = ((4369, 1, 1, 1, 15), (1, MAX_ROWS, 1, 1, 1))          # (B, H, W, L, NL)
HASH_PAST_BOUND = ((4096, 1, 1, 1, 16), (1, MAX_ROWS + 1, 1, 1, 1))

# ---- the census -----------------------------------------------------------------------------------------------------------------
NEW = "tests/test_gpu_launch_regimes.py"
TABLE = []


def _row(op, kernel, regime, where, condition, test, enters=None):
    """``enters``: a thunk that says whether the test's parameter list enters the regime: for every row of the new module (the
    lists above) and for the sweep rows of the op files (their own lists, read from their sources)."""
    TABLE.append(dict(op=op, kernel=kernel, regime=regime, where=where, condition=condition, test=test, enters=enters))


def _enters_sweep(op, regime, vector):
    return lambda: any(sweep_regime(wide_cv(op, C, sh)) == regime and (wide_cv(op, C, sh) != C) == vector for C, sh in wide_cases(op))


def old_list(path, name):
    """The tuple ``name`` of the op file ``path`` (a plain module constant), read from its source."""
    import ast
    import re
    with open(os.path.join(ROOT, path)) as f:
        m = re.search(rf"^{name} = (\(.*?\))", f.read(), re.M)
    return ast.literal_eval(m.group(1))


def _enters_sweep_before(test, name, regime, vector):
    """Whether the list ``name`` of the op file of ``test`` still holds a C whose sweep is in ``regime`` on that path (aligned
    tensors: C % 4 == 0 is the vector path with CV = C / 4); ``name`` None: the test's own literal C = 260 from unaligned tensors."""
    path = test.split("::")[0]
    if name is None:
        return lambda: "(16, 8), 260" in open(os.path.join(ROOT, path)).read() and sweep_regime(260) == regime and not vector
    return lambda: any(sweep_regime(C // 4 if vector else C) == regime for C in old_list(path, name) if (C % 4 == 0) == vector)


# who entered a sweep regime before this module: op -> {(vector, regime): (test, the list of C it runs)}
_T = {"interpolate": ("tests/test_gpu_interpolate.py::test_forward_bit_equal_to_restatement", "CS"),
      "texture": ("tests/test_gpu_texture.py::test_forward_bit_equal_to_restatement", "CS"),
      "texture_cube": ("tests/test_gpu_texture_cube.py::test_forward_bit_equal_to_restatement", "CS"),
      "texture_cube_mip": ("tests/test_gpu_texture_cube_mip.py::test_forward_bit_equal_to_restatement", "CS"),
      "texture_volume": ("tests/test_gpu_texture_volume.py::test_forward_and_gradients", "CS")}
_SWEEP_BEFORE = {op: {k: t for k in ((False, REGIMES[0]), (False, REGIMES[1])) + (() if op == "interpolate" else ((True, REGIMES[1]),))}
                 for op, t in _T.items()}
_SWEEP_BEFORE["texture_mip"] = {
    (False, REGIMES[0]): ("tests/test_gpu_texture_mip.py::test_channel_and_layer_grid", "GRID_CS"),
    (False, REGIMES[1]): ("tests/test_gpu_texture_mip.py::test_sampling_against_restatement", "CS"),
    (False, REGIMES[4]): ("tests/test_gpu_texture_mip.py::test_forward_with_more_channels_than_lanes", None),
    (True, REGIMES[0]): ("tests/test_gpu_texture_mip.py::test_channel_and_layer_grid", "GRID_CS"),
    (True, REGIMES[1]): ("tests/test_gpu_texture_mip.py::test_sampling_against_restatement", "CS")}
_SWEEP_WHERE = {
    "interpolate": ("k_interpolate", "dm2_interpolate.hip:k_interpolate", "IP_BLOCK", "C"),
    "texture": ("k_texture", "dm2_tex_core.h:tex_sweep", "TEX_BLOCK", "CV"),
    "texture_mip": ("k_texture_mip", "dm2_texture_mip.hip:k_texture_mip", "TEX_BLOCK", "CV"),
    "texture_cube": ("k_texture_cube", "dm2_tex_core.h:tex_sweep", "TEX_BLOCK", "CV"),
    "texture_cube_mip": ("k_texture_cube_mip", "dm2_texture_cube.hip:k_texture_cube_mip", "TEX_BLOCK", "CV"),
    "texture_volume": ("k_texture_volume", "dm2_tex_core.h:tex_sweep", "TEX_BLOCK", "CV"),
}
for _op in WIDE_OPS:
    _k, _where, _blk, _cv = _SWEEP_WHERE[_op]
    for _vec in (False,) if _op == "interpolate" else (False, True):
        for _reg in REGIMES:
            _before = _SWEEP_BEFORE[_op].get((_vec, _reg))
            _row(_op, f"{_k}<{'vector' if _vec else 'scalar'}>", f"sweep, {_reg}", _where,
                 f"const int dq = {_blk} / {_cv}, dr = {_blk} - dq * {_cv};",
                 _before[0] if _before else f"{NEW}::test_wide_channels",
                 _enters_sweep_before(*_before, _reg, _vec) if _before else _enters_sweep(_op, _reg, _vec))

# the vector / scalar selection of every launcher (``if (vec4)``): the op files' unaligned tests run both sides
for _op, _k, _where, _cond, _test in (
        ("interpolate", "k_interpolate_bwd_bary", "dm2_interpolate.hip:launch_interpolate_backward",
         "const bool vec4 = C % 4 == 0 && (((uintptr_t)attr | (uintptr_t)dL_dout) & 15) == 0;",
         "tests/test_gpu_interpolate.py::test_unaligned_tables_give_the_same_bits"),
        ("texture", "k_texture, k_texture_bwd_uv", "dm2_texture.hip:launch_texture, launch_texture_backward",
         "const bool vec4 = C % 4 == 0 && tex_aligned16(tex, out);", "tests/test_gpu_texture.py::test_unaligned_tables_give_the_same_bits"),
        ("texture_mip", "k_texture_mip", "dm2_texture_mip.hip:launch_texture_mip",
         "const bool vec4 = C % 4 == 0 && tex_aligned16(tex, out, mip);",
         "tests/test_gpu_texture_mip.py::test_unaligned_tensors_give_the_same_bits"),
        ("texture_cube", "k_texture_cube, k_texture_cube_bwd_dir", "dm2_texture_cube.hip:launch_texture_cube",
         "const bool vec4 = C % 4 == 0 && tex_aligned16(tex, out);", "tests/test_gpu_texture_cube.py::test_unaligned_tables_give_the_same_bits"),
        ("texture_cube_mip", "k_texture_cube_mip, k_texture_cube_mip_bwd_dir", "dm2_texture_cube.hip:launch_texture_cube_mip",
         "if (vec4)", "tests/test_gpu_texture_cube_mip.py::test_unaligned_views_give_the_same_bits"),
        ("texture_volume", "k_texture_volume, k_texture_volume_bwd_xyz", "dm2_texture_volume.hip:launch_texture_volume",
         "const bool vec4 = C % 4 == 0 && tex_aligned16(grid, out);",
         "tests/test_gpu_texture_volume.py::test_unaligned_and_strided_inputs_give_the_same_bits"),
        ("hash_grid", "k_hash_grid, k_hash_grid_bwd_xyz", "dm2_hash_grid.hip:launch_hash_grid",
         "const bool vec = F > 1 && (((uintptr_t)table | (uintptr_t)out) & align) == 0;",
         "tests/test_gpu_hash_grid.py::test_unaligned_and_strided_inputs_give_the_same_bits"),
        ("composite", "k_composite, k_composite_bwd", "dm2_composite.hip:launch_composite",
         "const bool vec4 = C % 4 == 0 && cp_aligned16(values, out, nullptr);",
         "tests/test_gpu_composite.py::test_unaligned_tensors_give_the_same_gradients")):
    _row(_op, _k, "vector and scalar reads", _where, _cond, _test)

# LVEC: four slots of a pixel at a time
_row("composite", "k_composite<.., LVEC, ..>", "LVEC = 4 and 1", "dm2_composite.hip:launch_composite",
     "const bool lvec = L > 0 && L % 4 == 0 && cp_aligned16(render_layers, per_face ? nullptr : alpha, nullptr);",
     "tests/test_gpu_composite.py::test_forward_bit_equal_to_restatement")
_row("coverage", "k_coverage<LVEC, MASK>", "LVEC = 4 and 1, with and without inside", "dm2_coverage.hip:launch_coverage",
     "const bool lvec = L % 4 == 0 && (((uintptr_t)render_layers | (uintptr_t)out_cov) & 15) == 0 && ((uintptr_t)inside & 3) == 0;",
     "tests/test_gpu_coverage_op.py::test_forward_bit_equal_to_restatement")
_row("cube_prefilter", "k_cube_prefilter<CH, OT, TR>", "faces up to and above PF_SPLIT_FACE", "dm2_cube_prefilter.hip:launch_cube_prefilter",
     "const int ot = z.n <= PF_SPLIT_FACE ? PF_SPLIT_TILE : PF_TILE;", "tests/test_gpu_cube_prefilter.py::test_many_tiles_sampled_rows")

# the scatters' channel chunks (DM2_TEX_CHUNK; interpolate's and the hash grid's own ladders)
for _op, _k, _where, _test in (
        ("interpolate", "k_interpolate_bwd_attr<CH>", "dm2_interpolate.hip:launch_interpolate_backward", "tests/test_gpu_interpolate.py::test_gradients_against_float64"),
        ("texture", "k_texture_bwd_tex<F, Bd, CH>", "dm2_texture.hip:launch_texture_backward", "tests/test_gpu_texture.py::test_every_instantiation_once"),
        ("texture_mip", "k_texture_mip_bwd_tex<Bd, CH>", "dm2_texture_mip.hip:launch_texture_mip_backward", "tests/test_gpu_texture_mip.py::test_every_instantiation_once"),
        ("texture_cube", "k_texture_cube_bwd_tex<F, CH>", "dm2_texture_cube.hip:launch_texture_cube_backward", "tests/test_gpu_texture_cube.py::test_every_instantiation_once"),
        ("texture_cube_mip", "k_texture_cube_mip_bwd_tex<CH>", "dm2_texture_cube.hip:launch_texture_cube_mip_backward",
         "tests/test_gpu_texture_cube_mip.py::test_gradients_against_float64"),
        ("texture_volume", "k_texture_volume_bwd_grid<F, Bd, CH>", "dm2_texture_volume.hip:launch_texture_volume_backward",
         "tests/test_gpu_texture_volume.py::test_forward_and_gradients")):
    _row(_op, _k, "chunk length CH = 1, 2, 3, 4 and a tail", _where, "DM2_TEX_CHUNK(C, " if _op != "interpolate" else "if (C == 1) DM2_IP_LAUNCH(1);", _test)
    _row(_op, _k, "chunk loop beyond 9 chunks (C > 36), the coordinate backward's channel loop with it",
         {"texture_mip": "dm2_tex_core.h:tex_scatter_layer", "texture_cube": "dm2_tex_core.h:tex_scatter_layer",
          "texture_cube_mip": "dm2_tex_core.h:tex_scatter_layer_masked", "texture_volume": "dm2_tex_core.h:tex_scatter_layer_masked"}.get(_op, _where),
         "for (int c0 = 0; c0 < C; c0 += CH)", f"{NEW}::test_wide_channels", lambda: min(SCALAR_CS + VECTOR_CS[1:]) > 36)
_row("hash_grid", "k_hash_grid<Fl, Bd, F, VEC>", "F = 1, 2, 4, 8", "dm2_hash_grid.hip:DM2_HG_F", "#define DM2_HG_F(F, X, ...)",
     "tests/test_gpu_hash_grid.py::test_forward_and_gradients")

# the hash grid's levels
_HG = "dm2_hash_grid.hip:hg_levels"
_HGC = "if (v < NL && (int64_t)R[v] * R[v] * R[v] <= (int64_t)T) lv.dense |= 1u << v;"


def _hash(pred):
    return lambda: any(pred(*hash_levels(N, q, NL, lg), NL, lg) for N, q, NL, lg, _ in HASH_CASES.values())


_row("hash_grid", "all three", "dense bits 0 .. 4 only, up to 6 levels", _HG, _HGC, "tests/test_gpu_hash_grid.py::test_forward_and_gradients")
_row("hash_grid", "all three", "32 levels (HG_MAX_LEVELS)", _HG, "for (int v = 0; v < HG_MAX_LEVELS; v++)", f"{NEW}::test_hash_grid_levels",
     _hash(lambda R, d, NL, lg: NL == 32))
_row("hash_grid", "all three", "a dense bit above bit 4, hashed levels above it", _HG, _HGC, f"{NEW}::test_hash_grid_levels",
     _hash(lambda R, d, NL, lg: d >> 5 != 0 and d != (1 << NL) - 1))
_row("hash_grid", "all three", "bit 31 of the dense word", _HG, _HGC, f"{NEW}::test_hash_grid_levels", _hash(lambda R, d, NL, lg: d >> 31 == 1))
_row("hash_grid", "all three", "the workload's layout: 16 levels, T = 2^19", _HG, _HGC, f"{NEW}::test_hash_grid_levels",
     _hash(lambda R, d, NL, lg: NL == 16 and lg == 19))
_row("hash_grid", "all three", "finest resolution 2^20, next to the 2^24 rule", "dm2_api.hip:check_hash_grid",
     'if (r > (1 << 20)) return fail("hash_grid: a hash grid\'s finest resolution must not exceed 2^20");',
     f"{NEW}::test_hash_grid_finest_level_at_its_limit", _hash(lambda R, d, NL, lg: R[-1] == 1 << 20))
_row("hash_grid", "all three", "log2(T) = 24, dense (R^3 == T) and hashed", "dm2_api.hip:check_hash_grid",
     'if (log2_rows < 4 || log2_rows > 24) return fail("hash_grid: a hash grid\'s log2(T) must be in 4..24");',
     f"{NEW}::test_hash_grid_largest_table", lambda: {hash_levels(N, q, NL, lg)[1] for N, q, NL, lg, _ in HASH_CASES.values() if lg == 24} == {0, 1})

# the grids: views and tile rows at their bounds
_SLOT = 'if ((S + 255) / 256 > 0x7FFFFFFF || views > 65535 || (H + dm2::TILE - 1) / dm2::TILE > 65535)'
for _op in SLOT_GRID_OPS:
    _chk = "dm2_api.hip:check_interpolate_sizes" if _op == "interpolate" else "dm2_api.hip:check_slot_grid"
    _cond = _SLOT if _op != "interpolate" else "|| B > 65535 || ((int64_t)H + dm2::TILE - 1) / dm2::TILE > 65535)"
    _row(_op, "the scatter's tile_grid(W, H, B)", "65535 views; 65535 tile rows", _chk, _cond, f"{NEW}::test_at_the_bound",
         lambda: AT_BOUND[0][0] == 65535 and (AT_BOUND[1][1] + 15) // 16 == 65535)
    _row(_op, "none", "one step past either bound: refused, nothing launched", _chk, _cond, f"{NEW}::test_one_step_past_the_bound",
         lambda: PAST_BOUND[0][0] == 65536 and (PAST_BOUND[1][1] + 15) // 16 == 65536)
_row("hash_grid", "k_hash_grid_bwd_table: dim3 blocks(tiles.x, tiles.y, NL * B)", "B * NL = 65535; 65535 tile rows", "dm2_api.hip:check_hash_grid",
     'return check_slot_grid("hash_grid", (int64_t)B * H * W * L, (int64_t)B * num_levels, H);', f"{NEW}::test_hash_grid_at_the_bound",
     lambda: HASH_AT_BOUND[0][0] * HASH_AT_BOUND[0][4] == 65535 and (HASH_AT_BOUND[1][1] + 15) // 16 == 65535)
_row("hash_grid", "none", "one step past either bound: refused, nothing launched", "dm2_api.hip:check_hash_grid",
     'return check_slot_grid("hash_grid", (int64_t)B * H * W * L, (int64_t)B * num_levels, H);', f"{NEW}::test_hash_grid_one_step_past_the_bound",
     lambda: HASH_PAST_BOUND[0][0] * HASH_PAST_BOUND[0][4] == 65536 and (HASH_PAST_BOUND[1][1] + 15) // 16 == 65536)
_COMP = "|| B > 65535 || ((int64_t)H + dm2::TILE - 1) / dm2::TILE > 65535)"
_row("composite", "k_composite_bwd<true, ..>: tile_grid(W, H, B)", "65535 views; 65535 tile rows", "dm2_api.hip:check_composite_sizes", _COMP,
     f"{NEW}::test_composite_at_the_bound", lambda: AT_BOUND[0][0] == 65535 and (AT_BOUND[1][1] + 15) // 16 == 65535)
_row("composite", "none", "one step past either bound: refused, nothing launched", "dm2_api.hip:check_composite_sizes", _COMP,
     f"{NEW}::test_composite_one_step_past_the_bound", lambda: PAST_BOUND[0][0] == 65536 and (PAST_BOUND[1][1] + 15) // 16 == 65536)
_COV = "if (B > 65535 || ((int64_t)H + dm2::TILE - 1) / dm2::TILE > 65535)"
_AT = lambda: AT_BOUND[0][0] == 65535 and (AT_BOUND[1][1] + 15) // 16 == 65535
_PAST = lambda: PAST_BOUND[0][0] == 65536 and (PAST_BOUND[1][1] + 15) // 16 == 65536
_row("coverage", "k_coverage, k_coverage_bwd: tile_grid(W, H, B)", "65535 views; 65535 tile rows", "dm2_api.hip:check_coverage_sizes", _COV,
     f"{NEW}::test_coverage_at_the_bound", _AT)
_row("coverage", "none", "one step past either bound: refused, nothing launched", "dm2_api.hip:check_coverage_sizes", _COV,
     f"{NEW}::test_coverage_one_step_past_the_bound", _PAST)
for _op, _where, _grid in (("shading_vectors", "dm2_api.hip:check_shading", "sh_grid: dim3(per_view / 256, 1, B)"),
                           ("bary_derivatives", "dm2_api.hip:dm2_bary_derivatives_window", "dim3 grid(per_view / 256, 1, B)")):
    _cond = f'if (B > 65535 || (per_view + 255) / 256 > 0x7FFFFFFF) return fail("{_op}: too many slots or views");'
    _row(_op, _grid, "65535 views (no bound on rows: the grid is flat per view)", _where, _cond, f"{NEW}::test_{_op}_at_the_bound",
         lambda: MAX_VIEWS == 65535)
    _row(_op, "none", "65536 views: refused, nothing launched", _where, _cond, f"{NEW}::test_{_op}_one_step_past_the_bound",
         lambda: MAX_VIEWS + 1 == 65536)
_MM = 'if (NB < 0 || NB > 65535) return fail("texture_mip: the number of textures must lie in [0, 65535]");'
_row("texture_mipmaps", "k_mip_level, k_mip_backward: tex_flat_grid(n, NB)", "65535 textures", "dm2_api.hip:check_mip_sizes", _MM,
     f"{NEW}::test_texture_mipmaps_at_the_bound", lambda: MAX_VIEWS == 65535)
_row("texture_mipmaps", "none", "65536 textures: refused, nothing launched", "dm2_api.hip:check_mip_sizes", _MM,
     f"{NEW}::test_texture_mipmaps_one_step_past_the_bound", lambda: MAX_VIEWS + 1 == 65536)
_row("cube_prefilter", "k_cube_prefilter: dim3 grid(6 * otiles * otiles, C / CH, cubes)", "10922 cubes taken, 10923 refused",
     "dm2_api.hip:cube_prefilter", 'if (cubes < 0 || cubes > 10922) return fail("cube_prefilter: the number of cubes must lie in [0, 10922]");',
     "tests/test_gpu_cube_prefilter.py::test_refusals_at_the_abi")

# Bounds on views or rows that this census leaves to their own files, and why.
OUT_OF_SCOPE = (
    ("dm2_forward_plan / dm2_forward_run / dm2_backward (check_render_desc), dm2_layers_* / dm2_rasterize_* (check_layers_desc), "
     "dm2_layers_composite* (check_composite_desc), dm2_prepare_faces* (check_prep_desc)",
     "not per-slot ops: they take descriptors of a scene (faces, vertices, cameras, scratch sized by a plan), and a frame of 65535 "
     "views or 2^20 rows needs a scene, a plan and an oracle run of that size; their grids are tile_grid(W, H, B) or (count / 256, "
     "B) under checks of tiles per axis and views that were read and found complete"),
)


def markdown():
    """The table as DESIGN.md prints it."""
    lines = ["| op | kernel | regime | selected by | test |", "|---|---|---|---|---|"]
    for r in TABLE:
        lines.append(f"| {r['op']} | `{r['kernel']}` | {r['regime']} | `{r['where']}` | `{r['test'].replace('tests/', '')}` |")
    return "\n".join(lines)
