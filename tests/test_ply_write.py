"""The host half of the scene export (include/gsr.h "scene export"): gsr_ply_write_host, the row
format, the raw (pre-activation) functions of gsr_detmath.h behind it, the argument errors of
all five new entry points and the temporary-file protocol.  No device: the device writer is
held to these bytes by tests/test_gpu_scene_save.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _oracle

INT32_MAX = 2 ** 31 - 1
QNAN = 0x7FC00000
NARRAYS = (38, 49, 59)
ROW = {38: 62, 49: 73, 59: 62}
A_OPACITY, A_SCALE0, A_SH0, A_TSCALE = 3, 4, 11, 39
# the arrays a reload must reproduce bit for bit: everything but what an activation touches
ACTIVATED = {38: [3, 4, 5, 6], 49: [3, 4, 5, 6, A_TSCALE], 59: [3, 4, 5, 6]}
# gsr_raw_log against float64, in ulp of the result: the sweep below measures 1.006 (on a
# subnormal; 0.722 over the normal floats), rounded up to the next whole ulp
B_LOG = 2.0


def ulp32(v):
    """The float32 spacing at |v| (v float64), as float64; the smallest normal's below it."""
    a = np.maximum(np.abs(np.asarray(v, np.float64)).astype(np.float32), np.float32(2.0 ** -126))
    return np.spacing(a).astype(np.float64)


def synthetic_soa(gsr, d, narrays, n, seed=5):
    p = os.path.join(str(d), f"synth{narrays}_{n}.ply")
    (gsr.write_synthetic_ply4d if narrays == 49 else gsr.write_synthetic_ply)(p, n, seed)
    return p, gsr.read_ply(p, four_d=narrays == 49, sh3=narrays == 59)


def split_file_bytes(data):
    cut = data.index(b"end_header\n") + len(b"end_header\n")
    return data[:cut], data[cut:]


def split_file(path):
    return split_file_bytes(open(path, "rb").read())


@pytest.fixture(scope="module")
def scenes(gsr, tmp_path_factory):
    """Per block kind: the synthetic SoA of 300 Gaussians, the file write_ply made of it and that
    file's rows."""
    d = tmp_path_factory.mktemp("ply_write")
    out = {}
    for na in NARRAYS:
        _, soa = synthetic_soa(gsr, d, na, 300)
        saved = os.path.join(str(d), f"saved{na}.ply")
        gsr.write_ply(saved, soa)
        rows = np.frombuffer(split_file(saved)[1], "<f4").reshape(300, ROW[na])
        out[na] = (soa, saved, rows)
    return out


# ------------------------------------------------------------------ header and size

@pytest.mark.parametrize("narrays", NARRAYS)
@pytest.mark.parametrize("n", [0, 1, 65])
def test_header_and_size(gsr, tmp_path, narrays, n):
    synth, soa = synthetic_soa(gsr, tmp_path, narrays, n)
    assert soa.shape == (narrays, n)
    out = str(tmp_path / "out.ply")
    gsr.write_ply(out, soa)
    header, body = split_file(out)
    assert header == split_file(synth)[0]
    assert gsr.ply_row_floats(narrays) == ROW[narrays]
    assert len(body) == n * ROW[narrays] * 4
    assert os.path.getsize(out) == len(header) + n * ROW[narrays] * 4


def test_row_format(gsr, scenes):
    """Every column of the rows against the table of include/gsr.h, per block kind."""
    for na in NARRAYS:
        soa, _, rows = scenes[na]
        bits = rows.view(np.uint32)

        def same(col, array):
            assert np.array_equal(bits[:, col], soa[array].view(np.uint32)), (na, col, array)

        for c in range(3):
            same(c, c)
            assert not bits[:, 3 + c].any()                      # nx ny nz: +0
            same(6 + c, A_SH0 + c)
            assert np.array_equal(bits[:, 55 + c], gsr.raw_probe(soa[A_SCALE0 + c], 0).view(np.uint32))
        for j in range(45):
            if na == 59:
                same(9 + j, A_SH0 + 3 * (1 + j % 15) + j // 15)
            elif j < 24:
                same(9 + j, A_SH0 + 3 + j)
            else:
                assert not bits[:, 9 + j].any()                  # +0, not -0
        assert np.array_equal(bits[:, 54], gsr.raw_probe(soa[A_OPACITY], 1).view(np.uint32))
        for c in range(4):
            same(58 + c, 7 + c)
        if na == 49:
            same(62, 38)
            assert np.array_equal(bits[:, 63], gsr.raw_probe(soa[A_TSCALE], 0).view(np.uint32))
            for c in range(9):
                same(64 + c, 40 + c)


# ------------------------------------------------------------------ round trip through the loader

@pytest.mark.parametrize("typed", [False, True], ids=["reference", "typed"])
@pytest.mark.parametrize("narrays", NARRAYS)
def test_round_trip(gsr, scenes, narrays, typed):
    soa, saved, rows = scenes[narrays]
    back = gsr.read_ply(saved, typed=typed, four_d=narrays == 49, sh3=narrays == 59)
    assert back.shape == soa.shape
    copied = [a for a in range(narrays) if a not in ACTIVATED[narrays]]
    assert np.array_equal(back[copied].view(np.uint32), soa[copied].view(np.uint32))
    if narrays == 38:   # what the block never held is written as 0: the full-SH reader sees zeros
        sh3 = gsr.read_ply(saved, typed=typed, sh3=True)
        for j in range(24, 45):
            assert not sh3[A_SH0 + 3 * (1 + j % 15) + j // 15].view(np.uint32).any(), j

    # The scales.  The file holds v = log s + dv with |dv| <= B_LOG ulp(v) (the sweep below); the
    # loader returns float(exp(double(v))) = s e^dv (1 + r), |r| <= 2^-24: a relative error of
    # |dv| + 2^-24 to first order, and 2^-23 covers the rounding and the second-order terms.
    for a, col in [(A_SCALE0 + c, 55 + c) for c in range(3)] + ([(A_TSCALE, 63)] if narrays == 49 else []):
        v = rows[:, col].astype(np.float64)
        s = soa[a].astype(np.float64)
        rel = np.abs(back[a].astype(np.float64) - s) / s
        bound = B_LOG * ulp32(v) + 2.0 ** -23
        print(f"narrays {narrays} array {a}: scale relative error {rel.max():.3g}, bound {bound.min():.3g}")
        assert (rel <= bound).all()

    # The opacity.  v = logit o + dv with |dv| <= B_LOG (ulp(log o) + ulp(log(1 - o))) + ulp(v) / 2
    # (the sweep below); d sigmoid / dv = o (1 - o), and 2^-24 is for the loader's own float
    # sigmoid (an exp, an add and a divide on values below 1).
    o = soa[A_OPACITY].astype(np.float64)
    v = rows[:, 54].astype(np.float64)
    dv = B_LOG * (ulp32(np.log(o)) + ulp32(np.log1p(-o))) + 0.5 * ulp32(v)
    err = np.abs(back[A_OPACITY].astype(np.float64) - o)
    bound = o * (1.0 - o) * dv + 2.0 ** -24
    print(f"narrays {narrays}: opacity error {err.max():.3g}, bound {bound.min():.3g}")
    assert (err <= bound).all()


# ------------------------------------------------------------------ the raw functions against float64

def log_sweep_inputs():
    """One value per mantissa step of 2^-12 in every binade, from the smallest subnormal to
    FLT_MAX (a subnormal binade has fewer than 2^12 values: then all of them)."""
    m = np.arange(4096, dtype=np.uint32) << np.uint32(11)
    parts = [(np.uint32(e) << np.uint32(23)) | m for e in range(1, 255)]
    for b in range(23):   # the subnormal binade [2^b, 2^(b+1)) of the bit pattern
        steps = np.unique((np.arange(4096, dtype=np.uint64) << np.uint64(b)) >> np.uint64(12)).astype(np.uint32)
        parts.append((np.uint32(1) << np.uint32(b)) | steps)
    parts.append(np.array([0x7F7FFFFF], np.uint32))
    return np.unique(np.concatenate(parts)).view(np.float32)


def test_raw_log_against_float64(gsr):
    x = log_sweep_inputs()
    assert x[0] == np.float32(1.401298464324817e-45) and x[-1] == np.finfo(np.float32).max and x.size > 10 ** 6
    got = gsr.raw_probe(x, 0).astype(np.float64)
    ref = np.log(x.astype(np.float64))
    err = np.abs(got - ref) / ulp32(ref)
    normal = x >= np.float32(2.0 ** -126)
    print(f"gsr_raw_log: {err.max():.4f} ulp over {x.size} values ({err[normal].max():.4f} over the normal ones, "
          f"worst at {x[err.argmax()]!r})")
    assert err.max() <= B_LOG
    assert got[x == 1.0] == 0.0


def test_raw_logit_against_float64(gsr):
    k = np.arange(1, 2 ** 24, dtype=np.float64)
    o32 = (k * 2.0 ** -24).astype(np.float32)
    o = o32.astype(np.float64)
    assert np.array_equal(o, k * 2.0 ** -24)                      # every k 2^-24 is a float
    got = gsr.raw_probe(o32, 1).astype(np.float64)
    l1, l2 = np.log(o), np.log1p(-o)                             # 1 - o is exact in float32 too
    ref = l1 - l2
    err = np.abs(got - ref)
    bound = B_LOG * (ulp32(l1) + ulp32(l2)) + 0.5 * ulp32(ref)
    print(f"gsr_raw_logit: absolute error {err.max():.3g}, {(err / bound).max():.3f} of its bound, "
          f"{(err / np.maximum(ulp32(l1), ulp32(l2))).max():.3f} ulp of the larger log")
    assert (err <= bound).all()
    assert got[2 ** 23 - 1] == 0.0 and not np.signbit(got[2 ** 23 - 1])   # o = 0.5


def bits_of(values):
    return np.asarray(values, np.float32).view(np.uint32)


def test_raw_specials_bit_for_bit(gsr):
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    tiny = np.array([1, 0x00400000, 0x007FFFFF], np.uint32).view(np.float32)   # subnormals
    payload = np.array([0x7FC12345, 0xFFC00001, 0x7F800001], np.uint32).view(np.float32)
    # gsr_raw_log
    x = np.concatenate([np.array([0.0, -0.0, inf, -inf, nan, -1.0, -1e-45], np.float32), payload])
    want = [0xFF800000, 0xFF800000, 0x7F800000, QNAN, QNAN, QNAN, QNAN, QNAN, QNAN, QNAN]
    assert gsr.raw_probe(x, 0).view(np.uint32).tolist() == want
    got = gsr.raw_probe(tiny, 0)
    scaled = gsr.raw_probe(tiny * np.float32(16777216.0), 0)      # exact scaling into the normal range
    assert np.array_equal(bits_of(got), bits_of(scaled - np.float32(16.635532)))
    assert np.abs(got.astype(np.float64) - np.log(tiny.astype(np.float64))).max() <= 1e-5
    # gsr_raw_logit
    x = np.concatenate([np.array([0.0, -0.0, 1.0, nan, 1.5, -0.25, np.nextafter(np.float32(1), inf), -1e-45, inf,
                                  -inf, 0.5], np.float32), payload])
    want = [0xFF800000, 0xFF800000, 0x7F800000, QNAN, QNAN, QNAN, QNAN, QNAN, QNAN, QNAN, 0, QNAN, QNAN, QNAN]
    assert gsr.raw_probe(x, 1).view(np.uint32).tolist() == want
    # a subnormal opacity and the largest one below 1 stay finite, as log o - log(1 - o)
    edge = np.array([tiny[0], tiny[2], 1.0 - 2.0 ** -24], np.float32)
    got = gsr.raw_probe(edge, 1)
    want = gsr.raw_probe(edge, 0) - gsr.raw_probe(np.float32(1.0) - edge, 0)
    assert np.array_equal(bits_of(got), bits_of(want)) and np.isfinite(got).all()
    assert abs(float(got[2]) - 24 * np.log(2.0)) < 1e-5


def test_specials_reload_as_themselves(gsr, tmp_path):
    """What the loader can have produced at the ends of the range comes back through -inf / +inf."""
    _, soa = synthetic_soa(gsr, tmp_path, 38, 4)
    soa[A_OPACITY] = [0.0, 1.0, 0.25, -0.0]
    soa[A_SCALE0] = [0.0, np.inf, 2.0, 1e-42]
    p = str(tmp_path / "ends.ply")
    gsr.write_ply(p, soa)
    back = gsr.read_ply(p)
    assert back[A_OPACITY].tolist() == [0.0, 1.0, 0.25, 0.0]
    assert back[A_SCALE0, :3].tolist() == [0.0, np.inf, 2.0]
    assert abs(float(back[A_SCALE0, 3]) / 1e-42 - 1.0) < 1e-2     # a subnormal: few bits to keep


# ------------------------------------------------------------------ the reference's own loader

def test_reference_loader_reads_a_saved_file(gsr, scenes, tmp_path):
    if not os.path.exists(_oracle.REF_DRIVER):
        pytest.skip("oracle/_ref/ref_driver not built (needs the reference sources at build time)")
    soa, saved, _ = scenes[38]
    out = str(tmp_path / "ref_soa.bin")
    subprocess.run([_oracle.REF_DRIVER, "ply", saved, out], check=True, stdout=subprocess.DEVNULL, timeout=60)
    raw = open(out, "rb").read()
    n = int(np.frombuffer(raw[:8], "<i8")[0])
    assert n == soa.shape[1]
    ref = np.frombuffer(raw[8:], "<f4").reshape(38, n)
    ours = np.zeros((38, n), np.float32)
    nn = ctypes.c_int64(-1)
    assert gsr.lib().gsr_ply_read_host(saved.encode(), ours.ctypes.data, n, ctypes.byref(nn)) == 0
    assert np.array_equal(ref.view(np.uint32), ours.view(np.uint32))


# ------------------------------------------------------------------ argument errors

def last_error(gsr):
    return gsr.lib().gsr_last_error().decode()


@pytest.fixture()
def host_args(gsr, tmp_path):
    """Arguments that pass every check of the two writers and of the pack, the "device"
    pointers being addresses inside a host buffer no refused call may touch."""
    buf = (ctypes.c_uint64 * 4096)()
    base = ctypes.addressof(buf)
    soa = np.zeros((59, 8), np.float32)
    return dict(buf=buf, scene=base, rows=base + 16384, soa=soa, path=str(tmp_path / "never.ply").encode())


WRITE_HOST = [
    (dict(path=None), "null pointer"),
    (dict(soa=None), "null pointer"),
    (dict(narrays=37), "narrays = 37"),
    (dict(narrays=0), "narrays = 0"),
    (dict(n=-1), "n = -1 out of range"),
    (dict(n=INT32_MAX + 1), f"n = {INT32_MAX + 1} out of range"),
]


@pytest.mark.parametrize("over,text", WRITE_HOST, ids=[t for _, t in WRITE_HOST])
def test_write_host_refuses(gsr, host_args, tmp_path, over, text):
    a = dict(path=host_args["path"], soa=host_args["soa"].ctypes.data, narrays=38, n=8)
    a.update(over)
    assert gsr.lib().gsr_ply_write_host(a["path"], a["soa"], a["narrays"], a["n"]) == -1
    assert last_error(gsr) == "gsr_ply_write_host: " + text
    assert os.listdir(tmp_path) == []                             # before any file work


SAVE = [
    (dict(scene=None), "null pointer"),
    (dict(path=None), "null pointer"),
    (dict(narrays=48), "narrays = 48"),
    (dict(n=-1), "n = -1 out of range"),
    (dict(n=INT32_MAX + 1), f"n = {INT32_MAX + 1} out of range"),
    (dict(chunk=-1), "chunk_rows = -1 < 0"),
]


@pytest.mark.parametrize("over,text", SAVE, ids=[t for _, t in SAVE])
def test_save_ply_refuses(gsr, host_args, tmp_path, over, text):
    a = dict(scene=host_args["scene"], narrays=38, n=8, path=host_args["path"], chunk=0)
    a.update(over)
    assert gsr.lib().gsr_scene_save_ply(a["scene"], a["narrays"], a["n"], a["path"], a["chunk"], None) == -1
    assert last_error(gsr) == "gsr_scene_save_ply: " + text
    assert os.listdir(tmp_path) == [] and not any(host_args["buf"])   # before any file or device work


PACK = [
    (dict(layout=1), "layout 1 is not a scene block"),            # AoS
    (dict(layout=4), "layout 4 is not a scene block"),
    (dict(layout=-1), "layout -1 is not a scene block"),
    (dict(n=-1), "n = -1 out of range"),
    (dict(n=INT32_MAX + 1), f"n = {INT32_MAX + 1} out of range"),
    (dict(first=-1), "rows [-1, -1 + 2) outside [0, 8)"),
    (dict(count=-1), "rows [3, 3 + -1) outside [0, 8)"),
    (dict(first=7), "rows [7, 7 + 2) outside [0, 8)"),
    (dict(first=9, count=0), "rows [9, 9 + 0) outside [0, 8)"),
    (dict(scene=None), "null pointer"),
    (dict(rows=None), "null pointer"),
    (dict(scene_off=2), "misaligned pointer"),
    (dict(rows_off=1), "misaligned pointer"),
    (dict(rows_off=2, count=0), "misaligned pointer"),
]


@pytest.mark.parametrize("over,text", PACK, ids=[f"{sorted(o.items())}" for o, _ in PACK])
def test_pack_rows_refuses(gsr, host_args, over, text):
    a = dict(scene=host_args["scene"], layout=0, n=8, first=3, count=2, rows=host_args["rows"])
    a.update({k: v for k, v in over.items() if not k.endswith("_off")})
    for k in ("scene", "rows"):
        if k + "_off" in over:
            a[k] += over[k + "_off"]
    rc = gsr.lib().gsr_scene_pack_rows(a["scene"], a["layout"], a["n"], a["first"], a["count"], a["rows"], None)
    assert rc == -1
    assert last_error(gsr) == "gsr_scene_pack_rows: " + text
    assert not any(host_args["buf"])


@pytest.mark.parametrize("layout", [0, 2, 3])
def test_pack_rows_of_nothing_needs_no_device(gsr, host_args, layout):
    L = gsr.lib()
    assert L.gsr_scene_pack_rows(host_args["scene"], layout, 8, 5, 0, host_args["rows"], None) == 0
    assert L.gsr_scene_pack_rows(host_args["scene"], layout, 8, 8, 0, None, None) == 0
    assert L.gsr_scene_pack_rows(None, layout, 0, 0, 0, None, None) == 0
    assert not any(host_args["buf"])


def test_row_floats_and_probe_refuse(gsr):
    L = gsr.lib()
    assert [L.gsr_ply_row_floats(na) for na in NARRAYS] == [62, 73, 62]
    for na in (0, 37, 39, 62, -38):
        assert L.gsr_ply_row_floats(na) == -1
        assert last_error(gsr) == f"gsr_ply_row_floats: narrays = {na}"
    x = np.ones(4, np.float32)
    y = np.full(4, 7.0, np.float32)
    for args in ((None, 4, 0, y.ctypes.data), (x.ctypes.data, 4, 0, None), (x.ctypes.data, -1, 0, y.ctypes.data),
                 (x.ctypes.data, 4, 2, y.ctypes.data), (x.ctypes.data, 4, -1, y.ctypes.data)):
        assert L.gsr_raw_probe(*args) == -1
        assert last_error(gsr) == "gsr_raw_probe: bad argument"
    assert (y == 7.0).all()
    assert L.gsr_raw_probe(x.ctypes.data, 0, 1, y.ctypes.data) == 0 and (y == 7.0).all()


# ------------------------------------------------------------------ the temporary file

def test_missing_directory_is_an_io_error(gsr, tmp_path):
    soa = np.zeros((38, 3), np.float32)
    path = tmp_path / "no_such_dir" / "out.ply"
    assert gsr.lib().gsr_ply_write_host(str(path).encode(), soa.ctypes.data, 38, 3) == -3
    assert last_error(gsr).startswith("gsr_ply_write_host: ")
    assert os.listdir(tmp_path) == []


def test_success_leaves_only_the_file(gsr, tmp_path, scenes):
    soa = scenes[38][0]
    out = tmp_path / "a.ply"
    gsr.write_ply(str(out), soa[:, :10])
    assert os.listdir(tmp_path) == ["a.ply"]
    ten = out.read_bytes()
    gsr.write_ply(str(out), soa[:, :4])                           # over an existing file
    assert os.listdir(tmp_path) == ["a.ply"]
    four = out.read_bytes()
    assert len(four) < len(ten) and split_file(str(out))[1] == split_file_bytes(ten)[1][:4 * 248]


def test_failed_write_keeps_the_old_file(gsr, tmp_path, scenes):
    """The data does not fit (a file size limit stands in for a full disk): GSR_E_IO, no
    temporary file left, and the file that was at `path` is as it was."""
    import resource
    soa = np.ascontiguousarray(scenes[38][0][:, :100])           # 24,800 bytes of rows
    out = tmp_path / "a.ply"
    out.write_bytes(b"the old file")
    soft, hard = resource.getrlimit(resource.RLIMIT_FSIZE)
    resource.setrlimit(resource.RLIMIT_FSIZE, (4096, hard))       # the interpreter ignores SIGXFSZ
    try:
        rc = gsr.lib().gsr_ply_write_host(str(out).encode(), soa.ctypes.data, 38, 100)
    finally:
        resource.setrlimit(resource.RLIMIT_FSIZE, (soft, hard))
    assert rc == -3
    assert last_error(gsr).startswith("gsr_ply_write_host: write to ")
    assert os.listdir(tmp_path) == ["a.ply"] and out.read_bytes() == b"the old file"
    gsr.write_ply(str(out), soa)                                  # and the same call succeeds afterwards
    assert os.path.getsize(out) == len(split_file(str(out))[0]) + 24800


def test_failed_rename_removes_the_temporary_file(gsr, tmp_path, scenes):
    """The rename fails (the destination is a directory that is not empty) after every row was
    written: GSR_E_IO, no temporary file left, the destination untouched."""
    soa = np.ascontiguousarray(scenes[38][0][:, :10])
    dest = tmp_path / "dest.ply"
    dest.mkdir()
    (dest / "keep.txt").write_text("still here")
    assert gsr.lib().gsr_ply_write_host(str(dest).encode(), soa.ctypes.data, 38, 10) == -3
    assert last_error(gsr).startswith("gsr_ply_write_host: renaming ")
    assert os.listdir(tmp_path) == ["dest.ply"]
    assert os.listdir(dest) == ["keep.txt"] and (dest / "keep.txt").read_text() == "still here"
