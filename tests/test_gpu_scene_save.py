"""The device half of the scene export (include/gsr.h "scene export"): Scene.save_ply and
Scene.pack_rows against the host writer, byte for byte.  tests/test_ply_write.py holds the host
writer to the row format and the loader; equality with it here carries the host / device parity
of the raw functions, the SH maps, the tile edges (64 rows), the chunk edges and the double
buffering."""
import os

import numpy as np
import pytest

from test_gpu_adam import ALL_LRS, zeros_like_groups
from test_gpu_parity import CAMS, cam_for
from test_gpu_scene_ops import dev, exact_renderer, frame, same_bits, soa_of_kind

pytestmark = pytest.mark.gpu

NARRAYS = (38, 49, 59)
SIZES = (0, 1, 63, 64, 65, 1000, 4097)      # 4097 rows x 73 floats: the largest file, 1.2 MB
CHUNKS = (0, 1, 64, 100, 257)
GUARD = 64
PATTERN = -1234.5


@pytest.fixture(scope="module")
def torch(gpu):
    import torch as t
    assert t.cuda.is_available()
    return t


@pytest.fixture(scope="module")
def soas(gpu, tmp_path_factory):
    """Per block kind the synthetic SoA of 4,097 Gaussians; the smaller scenes are its prefixes."""
    return {na: soa_of_kind(gpu, tmp_path_factory, na, max(SIZES)) for na in NARRAYS}


def host_bytes(gsr, d, soa):
    p = os.path.join(str(d), "host.ply")
    gsr.write_ply(p, soa)
    return open(p, "rb").read()


def block_bytes(gsr, torch, scene):
    """Every byte of the device block, header and padding included."""
    nbytes = gsr.lib().gsr_scene_bytes(scene.narrays, scene.n)
    buf = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    assert gsr.lib().gsr_scene_copy(buf.data_ptr(), scene.ptr, scene.narrays, scene.n, None) == 0
    torch.cuda.synchronize()
    return buf.cpu().numpy().tobytes()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("narrays", NARRAYS)
def test_save_equals_host_writer(gpu, torch, soas, tmp_path, narrays, n):
    soa = np.ascontiguousarray(soas[narrays][:, :n])
    scene = gpu.Scene.from_soa(soa)
    want = host_bytes(gpu, tmp_path, scene.download())
    assert len(want) == want.index(b"end_header\n") + 11 + 4 * n * gpu.ply_row_floats(narrays)
    before = block_bytes(gpu, torch, scene)
    out = str(tmp_path / "device.ply")
    for chunk in CHUNKS:
        scene.save_ply(out, chunk_rows=chunk)
        got = open(out, "rb").read()
        assert got == want, (narrays, n, chunk, len(got), len(want))
        os.remove(out)
        assert os.listdir(tmp_path) == ["host.ply"]               # no temporary file left
    assert block_bytes(gpu, torch, scene) == before              # the source is only read


def test_specials_on_the_device(gpu, torch, soas, tmp_path):
    """Opacities and scales at and beyond the ends of what the loader produces, planted across a
    tile edge: the device's raw functions give the host's bits (NaN bits included)."""
    n = 80
    soa = np.ascontiguousarray(soas[49][:, :n])
    sub = np.array([0x00000001, 0x00012345, 0x007FFFFF], np.uint32).view(np.float32)
    opacities = np.array([0.0, -0.0, 1.0, np.nan, 1.5, -0.25, sub[0], sub[1], sub[2], 1.0 - 2.0 ** -24, 0.5,
                          2.0 ** -24, np.inf, -np.inf], np.float32)
    scales = np.array([0.0, -0.0, sub[0], sub[1], sub[2], np.inf, np.nan, -1.0, -np.inf, 1.0, 2.0 ** -126,
                       np.finfo(np.float32).max], np.float32)
    soa[3, 58:58 + opacities.size] = opacities                    # rows 58..71: both sides of row 64
    soa[3, 0:opacities.size] = opacities[::-1]
    for a, at in ((4, 60), (5, 1), (6, 30), (39, 56)):            # the three scales and trbf_scale
        soa[a, at:at + scales.size] = scales
    weird_nan = np.array([0x7FC12345, 0xFFC00001, 0x7F800001], np.uint32).view(np.float32)
    soa[0, 3:6] = weird_nan                                       # payloads of copied arrays survive
    soa[3, 20:23] = weird_nan                                     # ... of activated ones become the quiet NaN
    scene = gpu.Scene.from_soa(soa)
    assert same_bits(scene.download(), soa)
    want = host_bytes(gpu, tmp_path, soa)
    out = str(tmp_path / "device.ply")
    for chunk in (0, 7):
        scene.save_ply(out, chunk_rows=chunk)
        assert open(out, "rb").read() == want
    rows = np.frombuffer(want[want.index(b"end_header\n") + 11:], "<u4").reshape(n, 73)
    assert rows[3:6, 0].tolist() == [0x7FC12345, 0xFFC00001, 0x7F800001]
    assert rows[20:23, 54].tolist() == [0x7FC00000] * 3
    assert rows[58:61, 54].tolist() == [0xFF800000, 0xFF800000, 0x7F800000]


WINDOWS = [(0, 200), (63, 2), (64, 64), (199, 1), (5, 0), (1, 130)]


@pytest.mark.parametrize("skew", [0, 1], ids=["aligned16", "aligned4"])
@pytest.mark.parametrize("narrays", NARRAYS)
def test_pack_rows_windows(gpu, torch, soas, tmp_path, narrays, skew):
    """Each window equals its slice of the whole pack, the whole pack equals the host writer's
    rows, and the guard words behind a window keep their pattern.  skew: the output starts one
    float off a 16-byte boundary (the 4-byte store path)."""
    n = 200
    P = gpu.ply_row_floats(narrays)
    soa = np.ascontiguousarray(soas[narrays][:, :n])
    scene = gpu.Scene.from_soa(soa)
    data = host_bytes(gpu, tmp_path, soa)
    whole = np.frombuffer(data[data.index(b"end_header\n") + 11:], "<u4").reshape(n, P)
    other = torch.cuda.Stream()
    for k, (first, count) in enumerate(WINDOWS):
        buf = torch.full((skew + count * P + GUARD,), PATTERN, dtype=torch.float32, device="cuda")
        out = buf[skew:]
        assert out.data_ptr() % 16 == 4 * skew
        torch.cuda.synchronize()                                  # the fill, before a pack on another stream
        scene.pack_rows(out, first, count, stream=other.cuda_stream if k % 2 else 0)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert np.array_equal(got[skew:skew + count * P].view(np.uint32).reshape(count, P), whole[first:first + count]), \
            (narrays, first, count)
        assert (got[:skew] == np.float32(PATTERN)).all() and (got[skew + count * P:] == np.float32(PATTERN)).all()


@pytest.mark.parametrize("narrays", NARRAYS)
def test_selected_block_saves_and_reloads(gpu, torch, soas, tmp_path, narrays):
    """A block Scene.select built (count 517, stride 576 != n): saved, it is the host writer's
    file of its download, and reloaded it is that file's own SoA."""
    n = 1000
    scene = gpu.Scene.from_soa(np.ascontiguousarray(soas[narrays][:, :n]))
    keep = np.zeros(n, np.uint8)
    keep[np.random.default_rng(narrays).permutation(n)[:517]] = 1
    picked = scene.select(dev(torch, keep))
    assert picked.n == 517
    before = block_bytes(gpu, torch, picked)
    want = host_bytes(gpu, tmp_path, picked.download())
    out = str(tmp_path / "picked.ply")
    picked.save_ply(out, chunk_rows=100)
    assert open(out, "rb").read() == want
    assert block_bytes(gpu, torch, picked) == before
    again = gpu.Scene.from_ply(out, sh3=narrays == 59)
    assert (again.narrays, again.n) == (narrays, 517)
    assert same_bits(again.download(), gpu.read_ply(out, four_d=narrays == 49, sh3=narrays == 59))


def test_save_is_ordered_on_its_stream(gpu, torch, soas, tmp_path):
    """adam_step, then save_ply, both queued on a non-default stream: the file holds the stepped
    values."""
    n = 4097
    scene = gpu.Scene.from_soa(np.ascontiguousarray(soas[38][:, :n]))
    unstepped = host_bytes(gpu, tmp_path, scene.download())
    rng = np.random.default_rng(9)
    g = {k: dev(torch, rng.normal(0, 1e-3, t.numel()).astype(np.float32))
         for k, t in zeros_like_groups(torch, n).items()}
    m, v = zeros_like_groups(torch, n), zeros_like_groups(torch, n)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    out = str(tmp_path / "stepped.ply")
    scene.adam_step(g, m, v, step=1, stream=s.cuda_stream, **ALL_LRS)
    scene.save_ply(out, chunk_rows=1000, stream=s.cuda_stream)
    got = open(out, "rb").read()
    s.synchronize()
    want = host_bytes(gpu, tmp_path, scene.download())
    assert got == want
    assert got != unstepped and len(got) == len(unstepped)


def test_the_loop_closes(gpu, orc, torch, tmp_path):
    """from_points -> adam_step -> save_ply -> Scene.from_ply: the reloaded scene renders through
    the exact blend exactly as the oracle renders read_ply of the saved file."""
    n, W, H = 400, 64, 64
    rng = np.random.default_rng(31)
    xyz = rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)
    rgb = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    scene = gpu.Scene.from_points(dev(torch, xyz), n, dev(torch, rgb), opacity=0.5, scale_mul=1.0)
    g = {k: dev(torch, rng.normal(0, 1e-2, t.numel()).astype(np.float32))
         for k, t in zeros_like_groups(torch, n).items()}
    m, v = zeros_like_groups(torch, n), zeros_like_groups(torch, n)
    scene.adam_step(g, m, v, step=1, **ALL_LRS)
    out = str(tmp_path / "trained.ply")
    scene.save_ply(out)
    assert os.listdir(tmp_path) == ["trained.ply"]
    soa = gpu.read_ply(out)
    assert soa.shape == (38, n) and np.isfinite(soa).all()
    reloaded = gpu.Scene.from_ply(out)
    assert (reloaded.narrays, reloaded.n) == (38, n)
    assert same_bits(reloaded.download(), soa)
    cam = cam_for(gpu, W, H, **CAMS[0])
    got = frame(gpu, torch, exact_renderer(gpu), reloaded, cam, W, H)
    assert same_bits(got, orc.render(soa, cam, W, H, 3.0))
    assert (got != 0).sum() > 1000
