"""CPU-only tests of the animated clips' host side: Utils.png.write_apng against a chunk parser written here from zlib /
struct (and against PIL where it is installed), its replace-when-complete file handling and argument errors, the
argument errors of rfn_hip.ops.compose_clip that need no GPU, the ABI of rfn_clip_compose_u8, and the SPREAD / MEAN rules
of the restatement (tests/clip_compose_ref.py) at known values."""
import ctypes
import os
import struct
import zlib

import numpy as np
import pytest
import torch

from tests.clip_compose_ref import compose_clip_ref, mean_rule, spread_rule


def parse_apng(blob):
    """(width, height, plays, [(delay_num, delay_den, pixels [H, W, 3])]) of an 8-bit RGB APNG whose frames are all full
    ones; asserts the signature, every CRC, the chunk order IHDR acTL (fcTL IDAT) (fcTL fdAT)* IEND, consecutive
    sequence numbers, the fcTL fields and filter type 0 on every line"""
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
    w, h, depth, colour, compression, filt, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, compression, filt, interlace) == (8, 2, 0, 0, 0)
    assert chunks[1][0] == b"acTL" and len(chunks[1][1]) == 8
    n_frames, plays = struct.unpack(">II", chunks[1][1])
    want = [b"IHDR", b"acTL", b"fcTL", b"IDAT"] + [b"fcTL", b"fdAT"] * (n_frames - 1) + [b"IEND"]
    assert [t for t, _ in chunks] == want
    assert chunks[-1][1] == b""
    seq, frames = 0, []
    for k in range(n_frames):
        (tag_c, ctl), (tag_d, data) = chunks[2 + 2 * k], chunks[3 + 2 * k]
        assert len(ctl) == 26
        s, fw, fh, x0, y0, num, den, dispose, blend = struct.unpack(">IIIIIHHBB", ctl)
        assert s == seq and (fw, fh, x0, y0, dispose, blend) == (w, h, 0, 0, 0, 0)
        seq += 1
        if k:
            assert struct.unpack(">I", data[:4])[0] == seq
            seq += 1
            data = data[4:]
        raw = zlib.decompress(data)
        assert len(raw) == h * (1 + 3 * w)
        lines = np.frombuffer(raw, dtype=np.uint8).reshape(h, 1 + 3 * w)
        assert not lines[:, 0].any(), "every line has filter type 0"
        frames.append((num, den, lines[:, 1:].reshape(h, w, 3)))
    return w, h, plays, frames


def _frames(t, h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(t, h, w, 3)).astype(np.uint8)


def _as_scanlines(px):
    t, h, w, _ = px.shape
    data = np.zeros((t, h, 1 + 3 * w), dtype=np.uint8)
    data[:, :, 1:] = px.reshape(t, h, 3 * w)
    return data


@pytest.mark.parametrize("scanlines", [False, True])
@pytest.mark.parametrize("h,w", [(1, 1), (9, 13)])
@pytest.mark.parametrize("t", [1, 3])
def test_write_apng_round_trip(tmp_path, t, h, w, scanlines):
    from Utils.png import write_apng
    px = _frames(t, h, w, 100 * t + h)
    data = _as_scanlines(px) if scanlines else px
    path = tmp_path / "a.png"
    got = write_apng(str(path), torch.from_numpy(data) if h == 9 else data, delay_ms=40 * t, loops=t - 1)
    assert got == (t, h, w)
    gw, gh, plays, frames = parse_apng(path.read_bytes())
    assert (gw, gh, plays, len(frames)) == (w, h, t - 1, t)
    for k, (num, den, f) in enumerate(frames):
        assert (num, den) == (40 * t, 1000)
        assert np.array_equal(f, px[k]), k
    assert os.listdir(tmp_path) == ["a.png"], "no temporary file remains"


@pytest.mark.parametrize("scanlines", [False, True])
@pytest.mark.parametrize("h,w", [(1, 1), (9, 13)])
@pytest.mark.parametrize("t", [1, 3])
def test_write_apng_is_read_by_pil(tmp_path, t, h, w, scanlines):
    Image = pytest.importorskip("PIL.Image")
    from Utils.png import write_apng
    px = _frames(t, h, w, 7 + t)
    write_apng(str(tmp_path / "a.png"), _as_scanlines(px) if scanlines else px, delay_ms=70, loops=2)
    with Image.open(str(tmp_path / "a.png")) as im:
        assert im.n_frames == t and im.info["loop"] == 2
        for k in range(t):
            im.seek(k)
            assert im.info["duration"] == pytest.approx(70.0)
            assert np.array_equal(np.asarray(im.convert("RGB")), px[k]), k


def test_write_apng_replaces_an_existing_file_and_leaves_no_temporary(tmp_path):
    from Utils.png import write_apng
    path = tmp_path / "s.png"
    path.write_bytes(b"not a png, and longer than the file that replaces it" * 100)
    px = _frames(2, 3, 4, 1)
    write_apng(str(path), px)
    assert all(np.array_equal(f, px[k]) for k, (_, _, f) in enumerate(parse_apng(path.read_bytes())[3]))
    write_apng(str(path), 255 - px)
    assert all(np.array_equal(f, 255 - px[k]) for k, (_, _, f) in enumerate(parse_apng(path.read_bytes())[3]))
    assert os.listdir(tmp_path) == ["s.png"]


def test_write_apng_failure_leaves_the_old_file_and_no_temporary(tmp_path, monkeypatch):
    from Utils import png
    path = tmp_path / "s.png"
    px = _frames(2, 3, 4, 2)
    png.write_apng(str(path), px)
    before = path.read_bytes()

    def boom(src, dst):
        raise OSError("disk full")
    monkeypatch.setattr(png.os, "replace", boom)
    with pytest.raises(OSError, match="disk full"):
        png.write_apng(str(path), 255 - px)
    assert path.read_bytes() == before
    assert os.listdir(tmp_path) == ["s.png"]


def test_write_apng_argument_errors(tmp_path):
    from Utils.png import write_apng
    p = str(tmp_path / "x.png")
    with pytest.raises(TypeError, match="uint8"):
        write_apng(p, np.zeros((2, 2, 2, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="pixels or .* scanlines"):
        write_apng(p, np.zeros((2, 2, 6), dtype=np.uint8))
    with pytest.raises(ValueError, match="pixels or .* scanlines"):
        write_apng(p, np.zeros((2, 7), dtype=np.uint8))          # one picture: write_png's input
    with pytest.raises(ValueError, match="filter type 0"):
        write_apng(p, np.ones((2, 2, 7), dtype=np.uint8))
    with pytest.raises(ValueError, match="at least one frame"):
        write_apng(p, np.zeros((0, 4, 4, 3), dtype=np.uint8))
    with pytest.raises(ValueError, match="at least one frame"):
        write_apng(p, np.zeros((2, 0, 4, 3), dtype=np.uint8))
    for kw in (dict(delay_ms=-1), dict(delay_ms=65536), dict(loops=-1)):
        with pytest.raises(ValueError, match="delay_ms"):
            write_apng(p, np.zeros((1, 2, 2, 3), dtype=np.uint8), **kw)
    assert os.listdir(tmp_path) == []


def test_compose_clip_argument_errors_without_a_gpu():
    from rfn_hip import ops
    Cell = ops.ClipCell
    f = torch.zeros(3, 1, 5, 7)
    g = torch.zeros(3, 4, 1, 5, 7)
    with pytest.raises(ValueError, match=r"cell \(0, 0\) is on cpu; the kernel needs device tensors \(no CPU fallback\)"):
        ops.compose_clip([[Cell(f), Cell(g, "mean"), None]], 3)
    with pytest.raises(TypeError, match="non-empty list of lists"):
        ops.compose_clip([], 3)
    with pytest.raises(TypeError, match="non-empty list of lists"):
        ops.compose_clip([Cell(f)], 3)
    with pytest.raises(ValueError, match="same number"):                       # a ragged grid
        ops.compose_clip([[Cell(f), Cell(f)], [Cell(f)]], 3)
    with pytest.raises(ValueError, match="same number"):
        ops.compose_clip([[]], 3)
    with pytest.raises(TypeError, match=r"cell \(0, 1\) must be a ClipCell or None, got Tensor"):
        ops.compose_clip([[Cell(f), f]], 3)
    with pytest.raises(TypeError, match=r"cell \(1, 0\) must be a float32 or uint8 tensor, got torch.float64"):
        ops.compose_clip([[Cell(f)], [Cell(f.double())]], 3)
    with pytest.raises(ValueError, match=r"mode of cell \(0, 0\)"):
        ops.compose_clip([[Cell(f, "median")]], 3)
    with pytest.raises(ValueError, match=r"cell \(0, 1\) \(mode 'mean'\) must be \[n, G, C, H, W\]"):   # no group dimension
        ops.compose_clip([[Cell(f), Cell(f, "mean")]], 3)
    with pytest.raises(ValueError, match=r"cell \(0, 0\) \(mode 'frame'\) must be \[n, C, H, W\]"):
        ops.compose_clip([[Cell(g)]], 3)
    with pytest.raises(ValueError, match=r"C in \{1, 3\}"):
        ops.compose_clip([[Cell(torch.zeros(3, 2, 5, 7))]], 3)
    with pytest.raises(ValueError, match=r"cell \(0, 1\) has frames \(1, 5, 8\), cell \(0, 0\) has \(1, 5, 7\)"):   # mixed shapes
        ops.compose_clip([[Cell(f), Cell(torch.zeros(3, 1, 5, 8))]], 3)
    with pytest.raises(ValueError, match=r"frames of cell \(0, 1\) must be dense CHW"):
        ops.compose_clip([[Cell(f), Cell(torch.zeros(3, 1, 5, 14)[..., ::2])]], 3)
    with pytest.raises(ValueError, match=r"frames of cell \(0, 0\) must be dense CHW"):
        ops.compose_clip([[Cell(torch.zeros(3, 4, 5, 7, 3).permute(0, 1, 4, 2, 3), "spread")]], 3)
    max_group, max_gain = ops.clip_limits()
    with pytest.raises(ValueError, match="has %d members, need 1..%d" % (max_group + 1, max_group)):
        ops.compose_clip([[Cell(torch.zeros(1, max_group + 1, 1, 1, 1), "spread")]], 3)
    with pytest.raises(ValueError, match="has 0 members"):
        ops.compose_clip([[Cell(torch.zeros(1, 0, 1, 1, 1), "mean")]], 3)
    for gain in (0, max_gain + 1):
        with pytest.raises(ValueError, match="gain of cell .* need 1..%d" % max_gain):
            ops.compose_clip([[Cell(g, "spread", gain=gain)]], 3)
    with pytest.raises(ValueError, match="`after` of cell"):
        ops.compose_clip([[Cell(f, after=(0, 0, 256))]], 3)
    with pytest.raises(ValueError, match="`before` of cell"):
        ops.compose_clip([[Cell(f, before=(0, 0))]], 3)
    with pytest.raises(ValueError, match="at least one cell with frames"):
        ops.compose_clip([[None, None]], 3)
    for kw in (dict(T=0), dict(zoom=0), dict(zoom=17), dict(border=-1), dict(border=65), dict(gutter=-1), dict(bg=256),
               dict(n_bits=0), dict(n_bits=9)):
        with pytest.raises(ValueError, match="need T >= 1"):
            ops.compose_clip([[Cell(f)]], **{"T": 3, **kw})
    # strides along n and G of any size are fine (views of [n, D, B, ...] and [B, T, ...]); the device check comes last
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.compose_clip([[Cell(torch.zeros(3, 4, 2, 1, 5, 7)[:, :, 1], "mean"),
                           Cell(torch.zeros(4, 3, 1, 5, 7, dtype=torch.uint8)[0])]], 3)
    assert ops.clip_shape(4, 11, 64, 64, 2, 2, 2) == (538, 1476)
    assert ops.clip_shape(2, 3, 5, 7, 1, 0, 0) == (10, 21)


def test_clip_abi_and_limits():
    """additive: the ABI number stays 2; the two limits of the header reach the binding through the library's queries;
    argument errors are answered before any launch (no GPU needed)"""
    from rfn_hip import lib, ops, pictures
    L = lib.load()
    assert L.rfn_abi_version() == lib.ABI_VERSION == 2
    assert lib.SIGNATURES["rfn_clip_compose_u8"] == [ctypes.c_void_p] + [ctypes.c_int] * 13 + [ctypes.c_long,
                                                                                                ctypes.c_void_p]
    header = open(lib.HEADER_PATH).read()
    assert "#define RFN_CLIP_MAX_GROUP (1024)" in header and "#define RFN_CLIP_MAX_GAIN (16)" in header
    assert ops.clip_limits() == (L.rfn_clip_max_group(), L.rfn_clip_max_gain()) == (1024, 16)
    assert pictures.compose_clip is ops.compose_clip and pictures.ClipCell is ops.ClipCell
    tab = (ctypes.c_longlong * 8)()
    #              R  N  T  C  H  W  zoom border gutter bg n_bits range_half lead
    good = [1, 1, 1, 1, 4, 4, 1, 0, 0, 255, 8, 1, 0]
    call = lambda a, table=ctypes.cast(tab, ctypes.c_void_p), out=256: L.rfn_clip_compose_u8(table, *a, out, None)
    bad = lambda **kw: [kw.get(k, v) for k, v in zip("R N T C H W zoom border gutter bg n_bits range_half lead".split(),
                                                     good)]
    for kw, code in ((dict(R=0), -1), (dict(N=0), -1), (dict(T=0), -1), (dict(H=0), -1), (dict(C=2), -2),
                     (dict(zoom=0), -3), (dict(zoom=17), -3), (dict(border=-1), -3), (dict(border=65), -3),
                     (dict(gutter=-1), -3), (dict(bg=256), -3), (dict(n_bits=0), -4), (dict(n_bits=9), -4),
                     (dict(lead=2), -4), (dict(W=2 ** 30), -5), (dict(T=2 ** 30), -5), (dict(gutter=2 ** 30), -5)):
        assert call(bad(**kw)) == code, kw
    assert b"C == 1 || C == 3" in (call(bad(C=2)), L.rfn_last_error())[1]
    assert call(good, table=None) == -6 and call(good, out=0) == -6


@pytest.mark.parametrize("members,gain,want", [((0, 255), 1, 127), ((0, 255), 2, 255), ((7, 7, 7), 16, 0),
                                               ((10, 12, 11, 13, 9), 4, 5)])
def test_spread_rule_at_known_values(members, gain, want):
    assert int(spread_rule(np.array(members).reshape(len(members), 1), gain)[0]) == want


def test_rules_against_float64():
    """SPREAD is gain x the population standard deviation of the bytes, rounded down and capped; MEAN rounds half up"""
    rs = np.random.RandomState(5)
    for _ in range(2000):
        G, gain = int(rs.randint(1, 12)), int(rs.randint(1, 17))
        b = rs.randint(0, 256, size=(G, 1))
        sd = gain * np.std(b.astype(np.float64))
        got = int(spread_rule(b, gain)[0])
        assert got == min(255, int(np.floor(sd + 1e-9))) or got == min(255, int(np.floor(sd - 1e-9))), (b.ravel(), gain)
        assert int(mean_rule(b)[0]) == int(np.floor(b.mean() + 0.5 + 1e-9))
    assert int(mean_rule(np.array([[1], [2]]))[0]) == 2 and int(mean_rule(np.array([[1], [2], [2]]))[0]) == 2


def test_restatement_layout():
    """the restatement itself on a grid small enough to read: sizes, gutter, ring colours on both sides of switch_at, the
    held last frame, zoom, an empty cell"""
    from rfn_hip import ops
    a = torch.arange(2 * 1 * 1 * 2, dtype=torch.uint8).reshape(2, 1, 1, 2) + 10   # frames (10, 11), (12, 13)
    cells = [[ops.ClipCell(a, switch_at=1, before=(1, 2, 3), after=(4, 5, 6)), None]]
    out = compose_clip_ref(cells, 3, zoom=2, border=1, gutter=1, bg=200)
    assert out.shape == (3, 6, 15, 3)
    assert (out[:, 0] == 200).all() and (out[:, :, 0] == 200).all() and (out[:, :, 7:] == 200).all()
    assert out[0, 1, 1].tolist() == [1, 2, 3] and out[1, 1, 1].tolist() == [4, 5, 6] and out[2, 4, 6].tolist() == [4, 5, 6]
    assert out[0, 2:4, 2:6, 0].tolist() == [[10, 10, 11, 11]] * 2
    assert out[1, 2:4, 2:6, 1].tolist() == [[12, 12, 13, 13]] * 2 and np.array_equal(out[2], out[1])
    lines = compose_clip_ref(cells, 3, zoom=2, border=1, gutter=1, bg=200, scanlines=True)
    assert lines.shape == (3, 6, 46) and not lines[:, :, 0].any() and np.array_equal(lines[:, :, 1:].reshape(out.shape), out)
