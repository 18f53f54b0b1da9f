"""CPU-only tests of the sample sheets' host side: Utils.png.write_png against a PNG decoder written here from zlib /
struct (and against PIL where it is installed), its replace-when-complete file handling, the argument errors of
rfn_hip.ops.compose_sheet that need no GPU, the ABI of rfn_sheet_compose_u8, and the --plot_every flag."""
import ctypes
import os
import struct
import zlib
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests.test_moving_mnist_host import _solver_argv


def decode_png(blob):
    """(IHDR fields, pixels [H, W, 3]) of an 8-bit RGB PNG; asserts signature, chunk order, every CRC, one IDAT and
    filter type 0 on every line"""
    assert blob[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(blob):
        n, tag = struct.unpack(">I4s", blob[pos:pos + 8])
        data = blob[pos + 8:pos + 8 + n]
        assert len(data) == n
        crc, = struct.unpack(">I", blob[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(tag + data) & 0xffffffff, "CRC of %r" % tag
        chunks.append((tag, data))
        pos += 12 + n
    assert pos == len(blob)
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    assert chunks[2][1] == b""
    w, h, depth, colour, compression, filt, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, compression, filt, interlace) == (8, 2, 0, 0, 0)
    raw = zlib.decompress(chunks[1][1])
    assert len(raw) == h * (1 + 3 * w)
    lines = np.frombuffer(raw, dtype=np.uint8).reshape(h, 1 + 3 * w)
    assert not lines[:, 0].any(), "every line has filter type 0"
    return (w, h), lines[:, 1:].reshape(h, w, 3)


def _pixels(h, w, seed):
    if h * w * 3 >= 256:   # every byte value occurs
        px = np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        px.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)
        return px
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


@pytest.mark.parametrize("scanlines", [False, True])
@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (330, 1322), (16, 16)])
def test_write_png_round_trip(tmp_path, h, w, scanlines):
    from Utils.png import write_png
    px = _pixels(h, w, h * 1000 + w)
    if (h, w) == (16, 16):
        px = np.arange(768, dtype=np.int64).reshape(16, 16, 3).astype(np.uint8)   # all 256 byte values, in order
        assert len(np.unique(px)) == 256
    data = px
    if scanlines:
        data = np.zeros((h, 1 + 3 * w), dtype=np.uint8)
        data[:, 1:] = px.reshape(h, 3 * w)
    path = tmp_path / "a.png"
    write_png(str(path), torch.from_numpy(data) if h == 5 else data)   # tensors and arrays alike
    (gw, gh), got = decode_png(path.read_bytes())
    assert (gw, gh) == (w, h)
    assert np.array_equal(got, px)
    assert os.listdir(tmp_path) == ["a.png"], "no temporary file remains"


@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (330, 1322)])
def test_write_png_is_read_by_pil(tmp_path, h, w):
    Image = pytest.importorskip("PIL.Image")
    from Utils.png import write_png
    px = _pixels(h, w, 7)
    write_png(str(tmp_path / "a.png"), px)
    with Image.open(str(tmp_path / "a.png")) as im:
        assert im.mode == "RGB"
        assert np.array_equal(np.asarray(im.convert("RGB")), px)


def test_write_png_replaces_an_existing_file_and_leaves_no_temporary(tmp_path):
    from Utils.png import write_png
    path = tmp_path / "s.png"
    path.write_bytes(b"not a png, and longer than the file that replaces it" * 100)
    px = _pixels(3, 4, 1)
    write_png(str(path), px)
    assert np.array_equal(decode_png(path.read_bytes())[1], px)
    write_png(str(path), 255 - px)
    assert np.array_equal(decode_png(path.read_bytes())[1], 255 - px)
    assert os.listdir(tmp_path) == ["s.png"]


def test_write_png_failure_leaves_the_old_file_and_no_temporary(tmp_path, monkeypatch):
    from Utils import png
    path = tmp_path / "s.png"
    px = _pixels(3, 4, 2)
    png.write_png(str(path), px)
    before = path.read_bytes()

    def boom(src, dst):
        raise OSError("disk full")
    monkeypatch.setattr(png.os, "replace", boom)
    with pytest.raises(OSError, match="disk full"):
        png.write_png(str(path), 255 - px)
    assert path.read_bytes() == before
    assert os.listdir(tmp_path) == ["s.png"]


def test_write_png_argument_errors(tmp_path):
    from Utils.png import write_png
    p = str(tmp_path / "x.png")
    with pytest.raises(TypeError, match="uint8"):
        write_png(p, np.zeros((2, 2, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="pixels or .* scanlines"):
        write_png(p, np.zeros((2, 6), dtype=np.uint8))
    with pytest.raises(ValueError, match="filter type 0"):
        write_png(p, np.ones((2, 7), dtype=np.uint8))
    with pytest.raises(ValueError, match="at least one pixel"):
        write_png(p, np.zeros((0, 4, 3), dtype=np.uint8))
    assert os.listdir(tmp_path) == []


def test_compose_sheet_argument_errors_without_a_gpu():
    from rfn_hip import ops
    f = torch.zeros(3, 1, 5, 7)
    with pytest.raises(ValueError, match=r"row 0 is on cpu; the kernel needs device tensors \(no CPU fallback\)"):
        ops.compose_sheet([f, f], 3)
    with pytest.raises(TypeError, match="row 1 must be a float32 or uint8 tensor, got torch.float64"):
        ops.compose_sheet([f, f.double()], 3)
    with pytest.raises(TypeError, match="row 0 must be a float32 or uint8 tensor, got list"):
        ops.compose_sheet([[1, 2]], 3)
    with pytest.raises(TypeError, match="non-empty list"):
        ops.compose_sheet([], 3)
    with pytest.raises(ValueError, match=r"row 1 has frames \(1, 5, 8\), row 0 has \(1, 5, 7\)"):
        ops.compose_sheet([f, torch.zeros(3, 1, 5, 8)], 3)
    with pytest.raises(ValueError, match=r"row 1 must be \[n, C, H, W\]"):
        ops.compose_sheet([f, torch.zeros(3, 5, 7)], 3)
    with pytest.raises(ValueError, match=r"C in \{1, 3\}"):
        ops.compose_sheet([torch.zeros(3, 2, 5, 7)], 3)
    with pytest.raises(ValueError, match="frames of row 1 must be dense CHW"):
        ops.compose_sheet([f, torch.zeros(3, 1, 5, 14)[..., ::2]], 3)
    with pytest.raises(ValueError, match="frames of row 0 must be dense CHW"):
        ops.compose_sheet([torch.zeros(3, 5, 7, 3).permute(0, 3, 1, 2)], 3)
    with pytest.raises(ValueError, match="row 0 holds 3 frames for 2 columns"):
        ops.compose_sheet([f], 2)
    with pytest.raises(ValueError, match="%d rows exceed the %d of one launch" % (ops.SHEET_MAX_ROWS + 1,
                                                                                    ops.SHEET_MAX_ROWS)):
        ops.compose_sheet([f] * (ops.SHEET_MAX_ROWS + 1), 3)
    for kw in (dict(gutter=-1), dict(bg=256), dict(n_bits=0), dict(n_bits=9)):
        with pytest.raises(ValueError, match="need n_cols >= 1"):
            ops.compose_sheet([f], 3, **kw)
    # a frame stride along n of any size is fine (a [T, B, ...] tensor's [:, 0]); the device check comes last
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.compose_sheet([torch.zeros(3, 4, 1, 5, 7)[:, 0], torch.zeros(4, 3, 1, 5, 7, dtype=torch.uint8)[0]], 3)
    assert ops.sheet_shape(5, 20, 64, 64, 2) == (332, 1322)


def test_sheet_abi():
    """additive: the ABI number stays 2; the row limit and the descriptor layout of the binding are the library's"""
    from rfn_hip import lib, ops
    L = lib.load()
    assert L.rfn_abi_version() == lib.ABI_VERSION == 2
    assert lib.SIGNATURES["rfn_sheet_compose_u8"] == [ctypes.c_void_p] + [ctypes.c_int] * 10 + [ctypes.c_long,
                                                                                                 ctypes.c_void_p]
    assert L.rfn_sheet_max_rows() == ops.SHEET_MAX_ROWS
    assert ctypes.sizeof(lib.rfn_sheet_row) == 24
    assert (lib.rfn_sheet_row.ptr.offset, lib.rfn_sheet_row.step.offset, lib.rfn_sheet_row.kind.offset,
            lib.rfn_sheet_row.count.offset) == (0, 8, 16, 20)
    # argument errors are answered before any launch (no GPU needed): a channel count other than 1 / 3, a bad count
    tab = (lib.rfn_sheet_row * 1)()
    tab[0].ptr, tab[0].step, tab[0].kind, tab[0].count = 256, 0, 1, 1
    call = lambda *a: L.rfn_sheet_compose_u8(ctypes.cast(tab, ctypes.c_void_p), *a, 256, None)
    assert call(1, 1, 2, 4, 4, 0, 255, 8, 1, 0) == -2
    assert b"C == 1 || C == 3" in L.rfn_last_error()
    assert call(1, 1, 1, 4, 4, -1, 255, 8, 1, 0) == -3
    assert call(1, 1, 1, 4, 4, 0, 256, 8, 1, 0) == -3
    assert call(1, 1, 1, 4, 4, 0, 255, 9, 1, 0) == -4
    assert call(ops.SHEET_MAX_ROWS + 1, 1, 1, 4, 4, 0, 255, 8, 1, 0) == -1
    tab[0].count = 2
    assert call(1, 1, 1, 4, 4, 0, 255, 8, 1, 0) == -8
    tab[0].count, tab[0].kind = 1, 2
    assert call(1, 1, 1, 4, 4, 0, 255, 8, 1, 0) == -7


def test_plot_every_flag_defaults_to_never():
    import main_rfn
    p = main_rfn.build_parser()
    assert p.parse_args([]).plot_every == 0
    assert p.parse_args(["--plot_every", "3"]).plot_every == 3


def test_namespace_without_the_flag_builds_a_solver(tmp_path, monkeypatch):
    """checkpoints written before --plot_every existed carry Namespaces without it"""
    import main_rfn
    from RFN.trainer import Solver
    rel = "/" + os.path.relpath(str(tmp_path), os.getcwd()) + "/"
    args = main_rfn.build_parser().parse_args(_solver_argv("--synthetic_data --choose_data mnist --path %s" % rel))
    old = Namespace(**{k: v for k, v in vars(args).items() if k != "plot_every"})
    assert not hasattr(old, "plot_every")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)   # host logic only: build on the CPU
    s = Solver(old)
    s.build()
    assert s.plot_counter == 0 and callable(s.plotter)
    assert os.listdir(s.path + "png_folder") == []
