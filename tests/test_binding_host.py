"""CPU-only tests of the derived binding (rfn_hip/lib.py): what the header parser refuses, the struct mirrors against
the header's typedefs and the sizes csrc asserts, the bytes of POPackPlan's descriptor table, ctypes refusing a value of
the wrong type, and the limits ops takes from the header."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rfn_hip.h")


def test_parser_refuses_an_unknown_type():
    from rfn_hip import lib
    sigs, res, consts = lib.parse_header("#define RFN_N 7\nint rfn_x(const float* p, long n);\nlong rfn_y(void);")
    assert sigs == {"rfn_x": [ctypes.c_void_p, ctypes.c_long], "rfn_y": []}
    assert res == {"rfn_x": ctypes.c_int, "rfn_y": ctypes.c_long} and consts == {"RFN_N": 7}
    with pytest.raises(RuntimeError, match=r"rfn_x.*const short\* p"):
        lib.parse_header("int rfn_x(const short* p);")
    with pytest.raises(RuntimeError, match=r"rfn_x.*short"):
        lib.parse_header("int rfn_x(int n, short k);")
    with pytest.raises(RuntimeError, match=r"rfn_x.*unsigned"):
        lib.parse_header("unsigned rfn_x(int n);")


def test_load_needs_the_header_copy(monkeypatch, tmp_path):
    from rfn_hip import lib
    assert os.path.samefile(os.path.dirname(lib.HEADER_PATH), os.path.dirname(lib.LIB_PATH))
    assert open(lib.HEADER_PATH).read() == open(HEADER).read()      # the build's copy is the header in include/
    monkeypatch.setattr(lib, "_lib", None)
    monkeypatch.setattr(lib, "HEADER_PATH", str(tmp_path / "rfn_hip.h"))
    with pytest.raises(RuntimeError, match="rfn_hip.h.*build it with"):
        lib.load()
    with pytest.raises(RuntimeError, match="build it with"):
        lib.SIGNATURES


def _header_structs():
    """typedef name -> [(field, C type)] of every struct typedef of include/rfn_hip.h"""
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;", txt, flags=re.S):
        fields = []
        for decl in m.group(1).split(";"):
            if decl.strip():
                first, *more = [d.strip() for d in decl.split(",")]
                ty, name = re.fullmatch(r"(.*[\s*])(\w+)", first).groups()
                assert "*" not in "".join(more)
                fields += [(n, " ".join(ty.split())) for n in [name] + more]
        out[m.group(2)] = fields
    return out


def test_struct_mirrors_match_the_header_typedefs():
    from rfn_hip import lib
    cmap = {"const float*": ctypes.c_void_p, "float*": ctypes.c_void_p, "const void*": ctypes.c_void_p,
            "int": ctypes.c_int, "long": ctypes.c_long}
    structs = _header_structs()
    assert set(structs) == set(lib.STRUCTS) == {"rfn_pack_desc", "rfn_po_pack_desc", "rfn_smallmap_pack_desc",
                                                "rfn_adam_entry", "rfn_sheet_row"}
    csrc = "".join(open(f).read() for f in sorted(glob.glob(os.path.join(ROOT, "recurrent-flows-msc_amd", "csrc", "*.hip"))))
    for name, fields in structs.items():
        mirror = lib.STRUCTS[name]
        assert mirror.__name__ == name
        assert [(n, cmap[ty]) for n, ty in fields] == list(mirror._fields_), name
        sizes = re.findall(r"static_assert\(sizeof\(%s\) == (\d+)," % name, csrc)
        assert len(sizes) == 1 and ctypes.sizeof(mirror) == int(sizes[0]), (name, sizes)
    assert [ctypes.sizeof(lib.STRUCTS[n]) for n in ("rfn_pack_desc", "rfn_po_pack_desc", "rfn_smallmap_pack_desc",
                                                    "rfn_adam_entry", "rfn_sheet_row")] == [32, 40, 40, 48, 24]


PO_RECORD = np.dtype([("w1", "<u8"), ("w2", "<u8"), ("w3", "<u8"), ("dst", "<u8"), ("Cin", "<i4"), ("C", "<i4")])


def _po_record_bytes(rows):
    rec = np.zeros(len(rows), dtype=PO_RECORD)
    for i, r in enumerate(rows):
        rec[i] = r
    return rec.view(np.uint8).tobytes()


def test_po_pack_plan_table_bytes():
    """the descriptor table of POPackPlan holds the bytes of the numpy record it was built from before: four <u8, two
    <i4, 40 bytes per net"""
    from rfn_hip import ops
    assert PO_RECORD.itemsize == 40
    rows = [(0x7f0012345600, 0x7f00deadbe00, 0x1000, 0xfffffffffff0, 14, 12), (256, 512, 768, 1024, 6, 4)]
    assert bytes(ops.POPackPlan.host_table(rows)) == _po_record_bytes(rows)
    # the plan itself, on two nets in host memory (nothing is launched): the forward and the backward table
    nets = [(torch.zeros(256, cin, 3, 3), torch.zeros(256, 256, 1, 1), torch.zeros(c, 256, 3, 3))
            for cin, c in ((14, 12), (38, 48))]
    plan = ops.POPackPlan(nets)
    want = [tuple(w.data_ptr() for w in n) + (b.data_ptr(), int(n[0].shape[1]), int(n[2].shape[0]))
            for n, b in zip(nets, plan.bufs)]
    assert plan.table.dtype == torch.uint8 and plan.table.numpy().tobytes() == _po_record_bytes(want)
    assert plan.n_bwd == 1 and plan.bwd_bufs[1] is None
    want_bwd = [tuple(w.data_ptr() for w in nets[0]) + (plan.bwd_bufs[0].data_ptr(), 14, 12)]
    assert plan.table_bwd.numpy().tobytes() == _po_record_bytes(want_bwd)


def test_a_value_of_the_wrong_type_is_refused_before_the_call():
    from rfn_hip import lib
    L = lib.load()
    with pytest.raises(ctypes.ArgumentError):
        L.rfn_wgrad_split_workgroups(1.5, 1, 8)
    with pytest.raises(ctypes.ArgumentError):
        L.rfn_wgrad_split_workgroups(None, 1, 8)
    assert L.rfn_wgrad_split_workgroups(1, 1, 8) == 1          # min(256 / tiles, G * n_stages / 8)
    assert L.rfn_wgrad_split_workgroups(True, 1, 8) == 1       # bool is an int


def test_limits_come_from_the_header():
    from rfn_hip import lib, ops
    defines = dict(re.findall(r"^#define (RFN_\w+) (\d+)$", open(HEADER).read(), flags=re.M))
    assert defines == {"RFN_INVCONV_MAX_STEPS": "32", "RFN_INVCONV_MAX_CHANNELS": "96", "RFN_SHEET_MAX_ROWS": "32"}
    assert lib.CONSTANTS == {k: int(v) for k, v in defines.items()}
    assert (ops.INVCONV_MAX_STEPS, ops.INVCONV_MAX_CHANNELS) == (32, 96)
    assert ops.SHEET_MAX_ROWS == 32 == lib.load().rfn_sheet_max_rows()
