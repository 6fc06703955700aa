"""The C-ABI library loads and exports every symbol include/dm2_hip.h declares (no compute calls)."""
import os
import re

from util import ROOT

from dmesh2_renderer_amd import _C


def declared_functions():
    hdr = open(os.path.join(ROOT, "include", "dm2_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(dm2_[a-z_0-9]+)\s*\(", hdr)))


def test_header_symbols_are_bound_and_exported():
    names = declared_functions()
    assert len(names) >= 9
    assert set(names) == set(_C.EXPORTS), (names, sorted(_C.EXPORTS))
    lib = _C.load_library()                       # raises if a declared symbol is missing
    for n in names:
        assert getattr(lib, n) is not None
    assert lib.dm2_abi_version() == _C.ABI_VERSION == int(re.search(r"#define DM2_ABI_VERSION (\d+)", open(os.path.join(ROOT, "include", "dm2_hip.h")).read()).group(1))
    assert _C.ABI_VERSION == 8


def test_one_symbol_per_operation():
    """ABI v7: an optional window, output or upstream gradient is a nullable argument of the operation's one symbol, not a
    symbol of its own.  v6 exported 62 symbols; the 16 that named another symbol plus one pointer are gone: 46.  ABI v8: an
    operation of its own has a symbol of its own, too.  The voxel grid, the hash grid, the cube's mip chain and the cube
    prefilter, which travelled as value codes of dm2_texture_cube, dm2_texture_mip and dm2_texture_mipmaps, got a forward and
    a backward export each: 54."""
    assert len(_C.EXPORTS) == 54
    # (these exist in one form only: their `_window` is part of the operation's name, no second symbol stands beside them)
    one_form = {"dm2_bary_derivatives_window", "dm2_shading_vectors_window", "dm2_shading_vectors_backward_window"}
    assert one_form <= set(_C.EXPORTS)
    for n in set(_C.EXPORTS) - one_form:
        assert not re.search(r"_(weights|inside)$", n), n
        assert not re.search(r"backward_(alpha|window)$", n), n
        assert not re.match(r"^dm2_(layers_plan|layers_run|rasterize\w*|coverage\w*|layers_composite\w*)_window$", n), n


def test_lookup_ops_share_no_export():
    """The six lookup records of the shim name six forward and six backward exports, and what the shim calls for one family of
    tests/shim_trace.py's OPS it calls for no other."""
    import json
    import shim_trace
    ops = [_C._TEXTURE, _C._TEXTURE_CUBE, _C._TEXTURE_VOLUME, _C._HASH_GRID, _C._TEXTURE_MIP, _C._TEXTURE_CUBE_MIP]
    assert sorted(op.name for op in ops) == sorted(shim_trace.OPS)
    assert len({op.forward for op in ops}) == len({op.backward for op in ops}) == 6
    assert len({op.forward for op in ops} | {op.backward for op in ops}) == 12
    for op in ops:
        assert op.forward in _C.EXPORTS and op.backward == op.forward + "_backward" and op.backward in _C.EXPORTS, op.name
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "lookup_shim_calls.json")))
    served = {}
    for case, rec in golden.items():
        family = max((n for n in shim_trace.OPS if case.startswith(n + "-")), key=len, default=None)
        if family is not None:
            for call in rec["calls"]:
                served.setdefault(call["export"], set()).add(family)
    assert set(served) == {op.forward for op in ops} | {op.backward for op in ops}
    assert all(len(f) == 1 for f in served.values()), served


def header_struct(name):
    """[(field, size, is_pointer)] of `typedef struct name {...} name;` in include/dm2_hip.h, in declaration order."""
    hdr = open(os.path.join(ROOT, "include", "dm2_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const\s+)?(\w+)\s*(\*?)\s*(.*)$", decl, flags=re.S)
        ctype, ptr, names = m.group(2), m.group(3) == "*", m.group(4)
        for nm in names.split(","):
            nm = nm.strip()
            is_ptr = ptr or nm.startswith("*")
            size = 8 if is_ptr else {"int32_t": 4, "float": 4, "int64_t": 8, "uint32_t": 4}[ctype]
            fields.append((nm.lstrip("* "), size, is_ptr))
    return fields


def test_structs_match_header_layout():
    """Field ORDER, sizes and offsets of the three descriptor structs and of dm2_window: the ctypes mirrors in _C.py against the declarations
    of include/dm2_hip.h (natural alignment, as the C compiler lays them out)."""
    import ctypes
    for name, cls in (("dm2_render_desc", _C.RenderDesc), ("dm2_layers_desc", _C.LayersDesc), ("dm2_prep_desc", _C.PrepDesc),
                      ("dm2_window", _C.Window)):
        decl = header_struct(name)
        assert [f[0] for f in decl] == [f[0] for f in cls._fields_], name
        off = 0
        for (nm, size, is_ptr), (cnm, ctype) in zip(decl, cls._fields_):
            off = (off + size - 1) // size * size
            cf = getattr(cls, cnm)
            assert (cf.offset, cf.size) == (off, size), (name, nm, cf.offset, off)
            assert (ctype is ctypes.c_void_p) == is_ptr, (name, nm)
            off += size
        assert ctypes.sizeof(cls) == (off + 7) // 8 * 8, name


def test_cpu_tensors_are_refused():
    import pytest
    import torch
    from util import soup_args
    args, _ = soup_args(32, 32, 10, 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.render_forward_cuda(*args)


def test_missing_library_fails_loudly(tmp_path):
    import pytest
    with pytest.raises(RuntimeError, match="native library not found"):
        _C.load_library(str(tmp_path / "nope.so"))
