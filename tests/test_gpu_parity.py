"""GPU parity: the HIP pipeline (through the C ABI) against the CPU oracle on
the same seeded inputs.  Integer / index outputs (AABBs, pixel centres, depth
keys, sort orders, tile ranges) must be bit-exact; the image gate is the
north-star per-pixel L-inf <= 1e-4.  The default blend (since round 4) is the
fast-exp one (GSR_TUNE_BLEND_EXP 1, include/gsr.h): it must composite exactly the
oracle's splats on every pixel (take maps, tests/test_gpu_fastexp.py) and stay within
FX_TOL (1e-5) of the oracle; the exact blend (GSR_TUNE_BLEND_EXP 0, environment
GSR_BLEND_EXP=0) is asserted bit-exact wherever a test selects it."""
import ctypes
import os

import numpy as np
import pytest

from conftest import LINF_TOL, ROOT, assert_frames, exact_blend, scene_soa  # noqa: F401

pytestmark = pytest.mark.gpu



@pytest.fixture(scope="module")
def torch(gpu):
    import torch as t
    assert t.cuda.is_available()
    return t


@pytest.fixture(scope="module")
def c1(gpu, tmp_path_factory):
    return scene_soa(gpu, tmp_path_factory, 10_000, 1)


def cam_for(gsr, W, H, pos=(0, 0, 4), look=(0, 0, 0), fov=50):
    return gsr.make_camera(position=pos, look_at=look, fov_y=fov, aspect=W / H)


def render_gpu(gsr, torch, scene, cam, W, H, k=3.0, tiling=None, renderer=None, layout=0, n=None, time=None):
    """One frame (rendered again while gsr_sync reports an overflow); time: of a 4D scene
    (None: the context's)."""
    r = renderer or gsr.Renderer()
    out = torch.empty(3 * W * H, dtype=torch.float32, device="cuda")
    for _ in range(3):
        rc = r.render(scene, cam, W, H, out.data_ptr(), k=k, tiling=tiling, layout=layout, n=n, time=time)
        if r.sync() == 0:
            break
    return out.view(3, H, W).cpu().numpy(), r


def assert_image_parity(got, want, exact=None):
    """L-inf gate; bit-exact for frames of the exact blend (conftest.assert_frames)."""
    return assert_frames(got, want, exact)


def test_math_probe_bitwise(gpu, orc):
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.uniform(-100, 90, 40000), rng.uniform(-4, 4, 40000),
                        rng.standard_normal(20000) * 1e3,
                        [0.0, -0.0, 0.5, -0.5, 1.5, 2.5, np.inf, -np.inf, np.nan, 1e-40, 88.7, -103.9]])
    y = np.concatenate([rng.uniform(-5, 5, 100000), np.ones(12)])
    y[y == 0] = 1.0
    xy = np.stack([x, y], 1).astype(np.float32)
    got = gpu.math_probe(xy)
    L = orc.lib()
    xs, ys = xy[:, 0], xy[:, 1]
    ref = np.zeros_like(got)
    ref[:, 0] = [L.orc_expf(v) for v in xs]
    ref[:, 8] = [L.orc_blend_expf(v) for v in xs]
    ref[:, 1] = [L.orc_sinf(v) for v in xs]
    ref[:, 2] = [L.orc_cosf(v) for v in xs]
    ref[:, 3] = [L.orc_atan2f(a, b) for a, b in zip(xs, ys)]
    with np.errstate(all="ignore"):
        ref[:, 4] = np.sqrt(xs)
        ref[:, 5] = xs / ys
        tr = np.trunc(xs)
        ref[:, 6] = np.where(np.abs(xs - tr) >= np.float32(0.5), tr + np.sign(xs), tr).astype(np.float32)
    same = (got.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(got) & np.isnan(ref))
    for col, name in [(0, "exp"), (1, "sin"), (2, "cos"), (3, "atan2"), (4, "sqrt"), (5, "div"), (6, "round"),
                      (8, "blend exp")]:
        bad = np.where(~same[:, col])[0]
        assert bad.size == 0, f"{name}: {bad.size} mismatches, e.g. x={xs[bad[:3]]} y={ys[bad[:3]]} got={got[bad[:3], col]} ref={ref[bad[:3], col]}"


KNOB_TILE_SPANS = 19
KNOB_BLEND_EXP = 22


def rect_pairs(want, order, W, H):
    """(tile << 32 | index) for every tile of every visible splat's tile rect, stable
    by tile over the depth order (the lists without tile row spans)."""
    tx, ty = (W + 15) // 16, (H + 15) // 16
    idx_sorted = (order & 0xFFFFFFFF).astype(np.int64)
    idx_sorted = idx_sorted[want["status"][idx_sorted] == 2]
    a = want["aabb"]
    ex_tiles = []
    for i in idx_sorted:
        x0, x1 = a[i, 0] // 16, min(tx - 1, a[i, 2] // 16)
        y0, y1 = a[i, 1] // 16, min(ty - 1, a[i, 3] // 16)
        for yy in range(y0, y1 + 1):
            for xx in range(x0, x1 + 1):
                ex_tiles.append((yy * tx + xx, i))
    ex = np.array(ex_tiles, dtype=np.uint64).reshape(-1, 2)
    ex_pairs = (ex[:, 0] << np.uint64(32)) | ex[:, 1]
    return ex_pairs[np.argsort(ex[:, 0], kind="stable")]


def max_alpha_on_tiles(want, pairs, W):
    """Largest alpha = op * exp(-md2 / 2) (float32, render.cu:329-332 operation order)
    of each (tile, splat) pair over the tile's pixels inside the splat's AABB."""
    tx = (W + 15) // 16
    tile = (pairs >> np.uint64(32)).astype(np.int64)
    idx = (pairs & np.uint64(0xFFFFFFFF)).astype(np.int64)
    a = want["aabb"][idx].astype(np.int64)
    best = np.full(pairs.size, -np.inf, np.float32)
    cx, cy = want["px_x"][idx].astype(np.float32), want["px_y"][idx].astype(np.float32)
    ic = want["inv_covar"][idx].astype(np.float32)
    op = want["opacity"][idx].astype(np.float32)
    for oy in range(16):
        for ox in range(16):
            px = (tile % tx) * 16 + ox
            py = (tile // tx) * 16 + oy
            ok = (px >= a[:, 0]) & (px <= a[:, 2]) & (py >= a[:, 1]) & (py <= a[:, 3])
            dx = px.astype(np.float32) - cx
            dy = py.astype(np.float32) - cy
            # gsr_blend_md2's fused multiply-adds: float32 products are exact in float64
            f64 = np.float64
            u = (ic[:, 0].astype(f64) * dx + (ic[:, 1] * dy)).astype(np.float32)
            v = (ic[:, 2].astype(f64) * dx + (ic[:, 3] * dy)).astype(np.float32)
            md = (dx.astype(f64) * u + (dy * v)).astype(np.float32)
            al = np.minimum(op * np.exp(np.float32(-0.5) * md), np.float32(0.99))
            best = np.where(ok, np.maximum(best, al), best)
    return best


CAMS = [dict(pos=(0, 0, 4)), dict(pos=(1.0, 0.5, 3.0), look=(0.2, 0, 0), fov=70), dict(pos=(0, 0, 1.5), fov=90),
        dict(pos=(-2.5, -1.0, -3.0))]


def temporally_culled(want, got):
    """The Gaussians of a 4D frame that the oracle's records (of orc.temporal's 3D scene, which
    has no temporal cull) keep visible and the 4D preprocess left without a tile."""
    return (want["status"] == 2) & (got["tile_count"] == 0)


def same_opacity_bits(got, want, nan_sign_free=False):
    """Record opacities bit for bit.  nan_sign_free: where both are NaN, the sign bit alone may
    differ.  A 3D record's opacity is the scene's own bits, but a 4D record's is computed, and
    the sign of a NaN that an operation makes (0 / 0 from dt = 0 and trbf_scale = 0) is left
    open by IEEE 754: 0 on gfx950, 1 on the x86-64 hosts of the oracle, flipped once more by
    the negation in exp(-(u u)).  Nothing reads it: alpha = fminf(NaN, 0.99) either way."""
    gb, wb = got.view(np.uint32), want.view(np.uint32)
    if nan_sign_free:
        both_nan = np.isnan(got) & np.isnan(want)
        gb, wb = np.where(both_nan, gb & 0x7FFFFFFF, gb), np.where(both_nan, wb & 0x7FFFFFFF, wb)
    return np.array_equal(gb, wb)


def check_preprocess_records(gpu, orc, soa, cam, W, H, k=3.0, pairs_of=rect_pairs, time=None, renderer=None):
    """The records, the depth order, tile_count, the pair list and the tile ranges of one frame
    without tile row spans, bit for bit against the oracle's records.  pairs_of: rect_pairs,
    or a faster statement of it for scenes of many pairs.  time: soa is a (49, n) 4D scene,
    preprocessed at `time` and held against the oracle's records of orc.temporal(soa, time);
    the Gaussians temporally_culled() names must then have no record, key or pair at all and
    every other one the oracle's (whether that set is the right one is the caller's to check,
    on `renderer`'s read_splats).  Returns the oracle's records."""
    scene = gpu.Scene.from_soa(soa)
    r = renderer or gpu.Renderer()
    r.set_tuning(KNOB_TILE_SPANS, 0)   # every tile of every rect (the spans test covers 1)
    r.preprocess(scene, cam, W, H, k=k, time=time)
    r.sort()
    got = r.read_splats(soa.shape[1])
    oracle = orc.preprocess(soa if time is None else orc.temporal(soa, time), cam, W, H, k)
    want = oracle
    if time is not None:
        want = oracle.copy()
        want["status"][temporally_culled(oracle, got)] = 0
    vis = want["status"] == 2
    assert vis.sum() > 0
    assert np.array_equal(got["tile_count"][~vis], np.zeros((~vis).sum(), np.uint32))
    assert (got["depth_key"][~vis] == 0xFFFFFFFF).all()
    g = got[vis]
    w = want[vis]
    assert np.array_equal(g["inv_covar"].view(np.uint32), w["inv_covar"].view(np.uint32))
    assert np.array_equal(g["color"].view(np.uint32), w["color"].view(np.uint32))
    assert same_opacity_bits(g["opacity"], w["opacity"], nan_sign_free=time is not None)
    assert np.array_equal(g["px_x"], w["px_x"]) and np.array_equal(g["px_y"], w["px_y"])
    assert np.array_equal(g["x_range"] & 0xFFFF, w["aabb"][:, 0]) and np.array_equal(g["x_range"] >> 16, w["aabb"][:, 2])
    assert np.array_equal(g["y_range"] & 0xFFFF, w["aabb"][:, 1]) and np.array_equal(g["y_range"] >> 16, w["aabb"][:, 3])
    assert np.array_equal(g["depth_key"], w["depth_key"])
    tx, ty = (W + 15) // 16, (H + 15) // 16
    tx0, tx1 = w["aabb"][:, 0] // 16, np.minimum(tx - 1, w["aabb"][:, 2] // 16)
    ty0, ty1 = w["aabb"][:, 1] // 16, np.minimum(ty - 1, w["aabb"][:, 3] // 16)
    assert np.array_equal(g["tile_count"], ((tx1 - tx0 + 1) * (ty1 - ty0 + 1)).astype(np.uint32))

    # depth order: stable by key, index tie-break
    order = r.read_depth_order(soa.shape[1])
    assert np.array_equal(order, orc.expected_depth_order(want))

    ex_pairs = pairs_of(want, order, W, H)
    pairs = r.read_pairs()
    assert r.pair_count() == ex_pairs.size
    assert np.array_equal(pairs, ex_pairs)
    ranges = r.read_tile_ranges()
    t_of = (ex_pairs >> np.uint64(32)).astype(np.int64)
    counts = np.bincount(t_of, minlength=tx * ty)
    nz = counts > 0
    assert np.array_equal((ranges[nz, 1] - ranges[nz, 0]).astype(np.int64), counts[nz])
    assert (ranges[~nz, 1] == ranges[~nz, 0]).all()
    return oracle


@pytest.mark.parametrize("ci", range(len(CAMS)))
def test_preprocess_records_bit_exact(gpu, orc, torch, c1, ci):
    path, soa = c1
    W, H = 640, 480
    check_preprocess_records(gpu, orc, soa, cam_for(gpu, W, H, **CAMS[ci]), W, H)


def check_tile_spans(gpu, orc, torch, soa, cam, W, H, k=3.0, floor=0.05, pairs_of=rect_pairs, time=None):
    """Tile row spans on against off over one frame (test_tile_spans_drop_only_unreachable_pairs).
    floor: the dropped share of the rect pairs must exceed it, so that spans that do nothing
    cannot pass.  time: soa is a (49, n) 4D scene rendered at `time`, against the oracle on
    orc.temporal(soa, time); the full list is then that of the Gaussians the 4D preprocess
    kept (temporally_culled() of the spans-off frame names the others).
    Returns (rect pairs, dropped pairs, largest alpha of a dropped pair)."""
    scene = gpu.Scene.from_soa(soa)
    soa3 = soa if time is None else orc.temporal(soa, time)
    # exact blend: the lists differ, so the fast blend's guard band (which counts list
    # entries) could re-blend different blocks; the exact images must be identical
    r_on, r_off = exact_blend(gpu.Renderer()), exact_blend(gpu.Renderer())
    assert r_on.get_tuning(KNOB_TILE_SPANS) == 2   # default: on up to 1.5M Gaussians
    r_on.set_tuning(KNOB_TILE_SPANS, 1)
    r_off.set_tuning(KNOB_TILE_SPANS, 0)
    with pytest.raises(gpu.GsrError):
        r_off.set_tuning(KNOB_TILE_SPANS, 3)
    got_on, _ = render_gpu(gpu, torch, scene, cam, W, H, k=k, renderer=r_on, time=time)
    got_off, _ = render_gpu(gpu, torch, scene, cam, W, H, k=k, renderer=r_off, time=time)
    assert np.array_equal(got_on.view(np.uint32), got_off.view(np.uint32))
    assert_image_parity(got_on, orc.render(soa3, cam, W, H, k), exact=True)
    want = orc.preprocess(soa3, cam, W, H, k)
    listed = want
    if time is not None:
        listed = want.copy()
        listed["status"][temporally_culled(want, r_off.read_splats(soa.shape[1]))] = 0
    full = pairs_of(listed, r_on.read_depth_order(soa.shape[1]), W, H)
    assert np.array_equal(r_off.read_pairs(), full)
    on = r_on.read_pairs()
    assert r_on.pair_count() == full.size          # pair_count: every tile of every rect
    kept = np.isin(full, on)
    assert np.array_equal(on, full[kept])          # a subsequence: same order, nothing new
    dropped = full[~kept]
    peak = max_alpha_on_tiles(want, dropped, W)
    print(f"rect pairs {full.size}, dropped {dropped.size} ({dropped.size / max(full.size, 1):.4f}), "
          f"largest alpha of a dropped pair {float(peak.max(initial=0.0)):.4e}")
    assert dropped.size > floor * full.size
    assert (peak < np.float32(1e-3)).all()
    # the row pass still makes one item per covered tile row
    spl = r_on.read_splats(soa.shape[1])
    ty = spl["tile_y_range"][spl["tile_count"] > 0]
    assert r_on.row_item_count() == int(((ty >> 16) - (ty & 0xFFFF) + 1).sum())
    return full.size, dropped.size, float(peak.max(initial=0.0))


@pytest.mark.parametrize("ci", range(len(CAMS)))
def test_tile_spans_drop_only_unreachable_pairs(gpu, orc, torch, c1, ci):
    """Tile row spans (GSR_TUNE_TILE_SPANS; the default 2 turns them on for this size): the tile lists are the full
    rect lists with some pairs left out, in the same order; every left-out pair is one
    whose splat reaches alpha < 1e-3 on every in-box pixel of that tile; the image is
    bit-identical to the one without spans and to the oracle's."""
    path, soa = c1
    W, H = 640, 480
    check_tile_spans(gpu, orc, torch, soa, cam_for(gpu, W, H, **CAMS[ci]), W, H)   # ~24 % dropped on config 2


@pytest.mark.parametrize("ci", range(len(CAMS)))
def test_image_config1_parity(gpu, orc, torch, c1, ci):
    path, soa = c1
    W, H = 640, 480
    cam = cam_for(gpu, W, H, **CAMS[ci])
    scene = gpu.Scene.from_soa(soa)
    got, _ = render_gpu(gpu, torch, scene, cam, W, H)
    want = orc.render(soa, cam, W, H, 3.0)
    assert (want != 0).sum() > 1000
    assert_image_parity(got, want)


@pytest.mark.parametrize("knobs", [{}, {13: 0}, {13: 1}, {13: 64}])
def test_blend_block_mappings_parity(gpu, orc, torch, c1, knobs):
    """Every block-to-workgroup mapping of the blend is bit-exact vs the oracle:
    13 = tiles per band (default 4; 0: one contiguous run per XCD), including frames
    small enough to fall back to one run per XCD.  The removed knobs are refused."""
    path, soa = c1
    scene = gpu.Scene.from_soa(soa)
    for W, H in ((640, 480), (333, 217), (37, 23), (1, 1)):
        cam = cam_for(gpu, W, H, **CAMS[1])
        r = gpu.Renderer()
        for kn, v in knobs.items():
            r.set_tuning(kn, v)
        got, _ = render_gpu(gpu, torch, scene, cam, W, H, renderer=r)
        assert_image_parity(got, orc.render(soa, cam, W, H, 3.0))
    r = gpu.Renderer()
    for kn in (12, 14, 15, 16, 17):
        with pytest.raises(gpu.GsrError):
            r.set_tuning(kn, 1)
    for v in (1, 2):
        with pytest.raises(gpu.GsrError):
            r.set_blend_variant(v)


BINNING_KNOBS = [{}, {8: 4, 9: 16}, {8: 16, 9: 4, 10: 7}, {31: 2048}, {31: 2048, 10: 7}, {31: 1024, 9: 16, 10: 7}]


def check_binning_matches_pair_sort(gpu, orc, torch, soa, cam, W, H, knobs, min_pairs=10_000):
    """One frame through the row + column binning with the given knobs and through the pair
    sort (knob 7 = 0), tile row spans off: the same pairs in the same order, the same image,
    the oracle's image (test_tile_binning_matches_pair_sort)."""
    scene = gpu.Scene.from_soa(soa)
    r_bin, r_sort = exact_blend(gpu.Renderer()), exact_blend(gpu.Renderer())
    for kn, v in knobs.items():
        r_bin.set_tuning(kn, v)
    r_bin.set_tuning(KNOB_TILE_SPANS, 0)   # the pair path lists every tile of every rect
    r_sort.set_tuning(7, 0)
    got_bin, _ = render_gpu(gpu, torch, scene, cam, W, H, renderer=r_bin)
    got_sort, _ = render_gpu(gpu, torch, scene, cam, W, H, renderer=r_sort)
    assert np.array_equal(got_bin.view(np.uint32), got_sort.view(np.uint32))
    pb, ps = r_bin.read_pairs(), r_sort.read_pairs()
    assert pb.shape == ps.shape and pb.shape[0] > min_pairs
    assert np.array_equal(pb, ps)
    assert_image_parity(got_bin, orc.render(soa, cam, W, H, 3.0), exact=True)
    # the row pass made one item per covered tile row of every visible splat
    spl = r_bin.read_splats(soa.shape[1])
    live = spl["tile_count"] > 0
    ty = spl["tile_y_range"][live]
    assert r_bin.row_item_count() == int(((ty >> 16) - (ty & 0xFFFF) + 1).sum())
    assert r_sort.row_item_count() == -1
    return pb


@pytest.mark.parametrize("knobs", BINNING_KNOBS)
def test_tile_binning_matches_pair_sort(gpu, orc, torch, c1, knobs):
    """Row + column binning (default for grids <= 256 x 256 tiles) gives the same
    tile lists as pair emission + the key-value tile sort: identical (tile,
    Gaussian) pairs in identical order, identical images, both equal to the
    oracle.  Knobs 8/9: items per thread of the row / column tiles (4, 16);
    10: column-pass workgroups (7 forces the grid-stride chunk loop); 31: row items
    per column-pass chunk (1024, the default at this size, or 2048)."""
    path, soa = c1
    W, H = 1000, 700
    check_binning_matches_pair_sort(gpu, orc, torch, soa, cam_for(gpu, W, H, pos=(0.4, 0.3, 3.5)), W, H, knobs)


def test_tile_binning_8bit_digits(gpu, orc, torch, c1):
    """More than 128 tiles per axis (2100 x 2060: 132 x 129 tiles): both binning
    scatters rank 8-bit digits; pairs and image equal the pair-sort path and the oracle."""
    path, soa = c1
    W, H = 2100, 2060
    scene = gpu.Scene.from_soa(soa)
    cam = cam_for(gpu, W, H, pos=(0.3, -0.2, 3.2), fov=60)
    r_bin, r_sort, r_span = (exact_blend(gpu.Renderer()) for _ in range(3))
    r_bin.set_tuning(KNOB_TILE_SPANS, 0)
    r_sort.set_tuning(7, 0)
    got, _ = render_gpu(gpu, torch, scene, cam, W, H, renderer=r_bin)
    ref, _ = render_gpu(gpu, torch, scene, cam, W, H, renderer=r_sort)
    spanned, _ = render_gpu(gpu, torch, scene, cam, W, H, renderer=r_span)
    tx, ty = r_bin.tile_grid()
    assert tx > 128 and ty > 128 and r_bin.row_item_count() > 0
    assert np.array_equal(r_bin.read_pairs(), r_sort.read_pairs())
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(spanned.view(np.uint32), ref.view(np.uint32))
    assert r_span.read_pairs().size < r_bin.read_pairs().size
    assert_image_parity(got, orc.render(soa, cam, W, H, 3.0))


def test_tile_binning_wide_frame_falls_back(gpu, orc, torch, c1):
    """More than 256 tile columns (W > 4096): the pair sort path renders it."""
    path, soa = c1
    W, H = 4200, 40
    scene = gpu.Scene.from_soa(soa)
    cam = cam_for(gpu, W, H)
    got, r = render_gpu(gpu, torch, scene, cam, W, H)
    assert r.tile_grid()[0] > 256
    want = orc.render(soa, cam, W, H, 3.0)
    assert (want != 0).sum() > 1000
    assert_image_parity(got, want)


@pytest.mark.parametrize("pos,look", [((0, 0, 4), (0, 0, 0)), ((0, 0, 17.3), (0, 0, 0)), ((0, 0, 4), (0, 0, 9))])
def test_depth_pass_plan_exact(gpu, orc, torch, c1, pos, look):
    """Trailing depth-sort passes are skipped on the device when they would be
    identities (camera at 4: keys < 2^24; at 17.3: keys straddle 2^24, no skip;
    looking away: everything culled).  The depth order must equal the full
    stable sort by (key, index) either way, and so must the image."""
    path, soa = c1
    W, H = 640, 480
    cam = cam_for(gpu, W, H, pos=pos, look=look)
    scene = gpu.Scene.from_soa(soa)
    want = orc.preprocess(soa, cam, W, H, 3.0)
    orders = []
    for skip in (1, 0):
        r = gpu.Renderer()
        r.set_tuning(gpu.TUNE_DEPTH_BUCKETS, 0)   # the LSD passes and their device plan
        r.set_tuning(6, skip)
        got, _ = render_gpu(gpu, torch, scene, cam, W, H, renderer=r)
        assert_image_parity(got, orc.render(soa, cam, W, H, 3.0))
        orders.append(r.read_depth_order(soa.shape[1]))
        keys = want["depth_key"][want["status"] == 2].astype(np.int64)
        if not skip:
            assert r.depth_passes() == 4
        elif keys.size == 0:
            assert r.depth_passes() == 1
        else:
            assert r.depth_passes() == (3 if keys.max() < (1 << 24) else 4)
    assert np.array_equal(orders[0], orc.expected_depth_order(want))
    assert np.array_equal(orders[0], orders[1])


@pytest.mark.parametrize("items", [4, 8, 16])
def test_depth_sort_carries_rects(gpu, orc, torch, c1, items):
    """The depth sort carries every Gaussian's packed 4-B tile rect through its passes
    (read at the item's position on a fresh frame, gathered by index when the same
    frame is sorted again, since its items are then in a pass's order).  Every tile
    size (4, 8, 16 items per thread) and the repeated sort give the first sort's tile
    lists and the oracle's image; gsr_get_tuning reads the knob back."""
    path, soa = c1
    W, H = 640, 480
    cam = cam_for(gpu, W, H, **CAMS[1])
    scene = gpu.Scene.from_soa(soa)
    r = gpu.Renderer()
    assert r.get_tuning(2) == 0
    r.set_tuning(2, items)
    assert r.get_tuning(2) == items
    got, _ = render_gpu(gpu, torch, scene, cam, W, H, renderer=r)
    want = orc.render(soa, cam, W, H, 3.0)
    assert_image_parity(got, want)
    first = r.read_pairs()
    assert first.shape[0] > 10_000
    r.sort()
    assert np.array_equal(r.read_pairs(), first)
    out = torch.empty(3 * W * H, dtype=torch.float32, device="cuda")
    r.blend(out.data_ptr())
    assert r.sync() == 0
    assert_image_parity(out.view(3, H, W).cpu().numpy(), want)


def test_tuning_defaults_read_back(gpu):
    """gsr_get_tuning returns the documented defaults (include/gsr.h) and what
    gsr_set_tuning set; unknown knobs are refused."""
    r = gpu.Renderer()
    defaults = {1: 16, 2: 0, 3: 1024, 4: 0, 5: 1, 6: 1, 7: 1, 8: 4, 9: 8, 10: 0, 11: 1, 13: 4, 18: 2, 19: 2,
                23: 2, 24: 250, 31: 0}
    for kn, v in defaults.items():
        assert r.get_tuning(kn) == v, kn
    r.set_tuning(9, 16)
    assert r.get_tuning(9) == 16
    r.set_tuning(31, 2048)
    assert r.get_tuning(31) == 2048
    with pytest.raises(gpu.GsrError):
        r.set_tuning(31, 512)
    with pytest.raises(gpu.GsrError):
        r.get_tuning(12)


def test_depth_pass_budget_adapts_and_recovers(gpu, orc, torch, c1):
    """The binning path launches only the depth passes recent frames needed (4 checked
    frames needing 3 lower the budget to 3).  A frame whose keys then need 4 (camera
    at 17.3: keys straddle 2^24) is flagged — gsr_sync reports an overflow — and its
    re-render runs all four passes, bit-exact against the oracle."""
    path, soa = c1
    W, H = 640, 480
    scene = gpu.Scene.from_soa(soa)
    near = cam_for(gpu, W, H, pos=(0, 0, 4))
    far = cam_for(gpu, W, H, pos=(0, 0, 17.3))
    r = gpu.Renderer()
    r.set_tuning(gpu.TUNE_DEPTH_BUCKETS, 0)       # the LSD passes' budget (the bucket sort has none)
    out = torch.empty(3 * W * H, dtype=torch.float32, device="cuda")
    for i in range(8):
        r.render(scene, near, W, H, out.data_ptr())
        assert r.sync() == 0 or i == 0
        assert r.depth_passes() == 3
    assert_image_parity(out.view(3, H, W).cpu().numpy(), orc.render(soa, near, W, H, 3.0))
    r.render(scene, far, W, H, out.data_ptr())
    assert r.sync() != 0                      # launched 3, needed 4: flagged
    r.render(scene, far, W, H, out.data_ptr())
    assert r.sync() == 0 and r.depth_passes() == 4
    assert_image_parity(out.view(3, H, W).cpu().numpy(), orc.render(soa, far, W, H, 3.0))


def test_blend_slow_path_and_degenerate_records(gpu, orc, torch, c1):
    """Records without the blend's fast-path proof (cull word S = inf: needle-thin
    Gaussians whose conic is not robustly positive definite and has coefficients
    ~1e7) and records with NaN opacity (md2 cutoff NaN: never culled; alpha =
    fminf(NaN, 0.99)) run the exact one-splat path; the image must still equal the
    oracle bit for bit, and the diagnostics must show the slow path ran."""
    path, soa = c1
    s = soa.copy()
    rng = np.random.default_rng(7)
    n = s.shape[1]
    thin = rng.choice(n, 300, replace=False)
    s[4, thin] = 1e-6                       # scale0: needle along one axis
    s[5, thin] = 0.05
    s[6, thin] = 0.05
    nan_op = rng.choice(np.setdiff1d(np.arange(n), thin), 40, replace=False)
    s[3, nan_op] = np.nan
    W, H = 640, 480
    cam = cam_for(gpu, W, H)
    want = orc.render(s, cam, W, H, 3.0)
    for _ in range(1):
        r = gpu.Renderer()
        got, _ = render_gpu(gpu, torch, gpu.Scene.from_soa(s), cam, W, H, renderer=r)
        assert_image_parity(got, want)
        r.set_diagnostics(True)
        got2, _ = render_gpu(gpu, torch, gpu.Scene.from_soa(s), cam, W, H, renderer=r)
        assert_image_parity(got2, want)
        d = r.blend_counters_ex()
        assert d["slow_path_iters"] > 0
        # the fast blend hands every block holding such a record to the exact blend
        assert (d["reblended_blocks"] > 0) != (r.get_tuning(KNOB_BLEND_EXP) == 0)
        r.set_tuning(KNOB_BLEND_EXP, 0)
        got3, _ = render_gpu(gpu, torch, gpu.Scene.from_soa(s), cam, W, H, renderer=r)
        assert_image_parity(got3, want, exact=True)


@pytest.mark.parametrize("ci", [0, 1, 3])
def test_sh3_mode_parity(gpu, orc, torch, c1, ci):
    """Opt-in "Inria-correct" SH-3 scenes (degree-3 colour, channel-major f_rest)
    against the oracle's independent restatement, bit-exact; the colours differ
    from the reference-mode render of the same file (sanity)."""
    path, soa = c1
    W, H = 640, 480
    cam = cam_for(gpu, W, H, **CAMS[ci])
    scene = gpu.Scene.from_ply(path, sh3=True)
    assert scene.is_sh3
    got, r = render_gpu(gpu, torch, scene, cam, W, H)
    soa3 = orc.ply_read_sh3(path)
    with orc.sh3_mode():
        want = orc.render(soa3, cam, W, H, 3.0)
        want_spl = orc.preprocess(soa3, cam, W, H, 3.0)
    assert_image_parity(got, want)
    vis = want_spl["status"] == 2
    g = r.read_splats(soa.shape[1])[vis]
    assert np.array_equal(g["color"].view(np.uint32), want_spl["color"][vis].view(np.uint32))
    assert not np.array_equal(got, orc.render(soa, cam, W, H, 3.0))
    # the drop-in recognises an SH-3 block from its header
    t = gpu.TilingInformation(50, 50, H, W)
    host = gpu.preprocessCUDAGaussians(scene.ptr, scene.n, cam, t.num_tile_y, t.num_tile_x, t.width_stride,
                                       t.height_stride, W, H, 3.0)
    assert_image_parity(host, want)


def test_dropin_scene_block_reference_tiling(gpu, orc, torch, c1):
    """loadGaussianCudaFromPly + preprocessCUDAGaussians (the viewer's calls),
    reference 50x50 tiling (cull_sort_test.cpp:44-45)."""
    path, soa = c1
    W, H = 640, 480
    ptr, n = gpu.loadGaussianCudaFromPly(path)
    assert ptr and n == 10_000
    t = gpu.TilingInformation(50, 50, H, W)
    cam = cam_for(gpu, W, H)
    got = gpu.preprocessCUDAGaussians(ptr, n, cam, t.num_tile_y, t.num_tile_x, t.width_stride, t.height_stride,
                                      W, H, 3.0)
    want = orc.render(soa, cam, W, H, 3.0, tiling=(50, 50, t.width_stride, t.height_stride))
    assert_image_parity(got, want)
    gpu.lib().gsr_scene_free(ptr)


def aos_records(soa):
    n = soa.shape[1]
    rec = np.zeros((n, 60), dtype=np.float32)           # 240 B (gaussians.hpp:16-30)
    rec[:, 0:3] = soa[0:3].T                            # x, y, z
    rec[:, 6:33] = soa[11:38].T                         # sh[27]
    rec[:, 36] = soa[3]                                 # opacity
    rec[:, 37:40] = soa[4:7].T                          # scale
    rec[:, 40:44] = soa[7:11].T                         # rot
    rec[:, 3:6] = 7.0                                   # normals: ignored
    rec[:, 33:36] = -1.0                                # color: recomputed
    return rec


@pytest.mark.parametrize("n", [4000, 2, 1])
def test_dropin_aos_input(gpu, orc, torch, c1, n):
    """A reference-layout Gaussian[] device array (e.g. from the reference's own loader).
    One and two records: the layout probe reads 16 B first when the whole 256-B header
    would run past a 240-B array, one 256-B read otherwise."""
    path, soa = c1
    W, H = 320, 240
    cam = cam_for(gpu, W, H, pos=(0.3, 0.2, 3.5))
    if n < 10:   # splats in view, so the tiny images are not trivially empty
        spl = orc.preprocess(soa, cam, W, H, 3.0)
        vis = np.nonzero(spl["status"] == 2)[0]
        sub = soa[:, vis[:n]]
    else:
        sub = soa[:, :n]
    rec = aos_records(sub)
    dev = torch.from_numpy(rec).cuda()
    t = gpu.TilingInformation(40, 40, H, W)
    got = gpu.preprocessCUDAGaussians(dev.data_ptr(), n, cam, t.num_tile_y, t.num_tile_x, t.width_stride,
                                      t.height_stride, W, H, 3.0)
    torch.cuda.synchronize()
    want = orc.render(sub, cam, W, H, 3.0, tiling=(40, 40, t.width_stride, t.height_stride))
    assert (want != 0).any()
    assert_image_parity(got, want)
    # the same splats as a one- or two-Gaussian scene block through the drop-in
    if n < 10:
        scene = gpu.Scene.from_soa(np.ascontiguousarray(sub))
        got2 = gpu.preprocessCUDAGaussians(scene.ptr, n, cam, t.num_tile_y, t.num_tile_x, t.width_stride,
                                           t.height_stride, W, H, 3.0)
        assert_image_parity(got2, want)


@pytest.mark.parametrize("tiling", [(8, 8, 40, 30), (7, 3, 92, 160), (3, 5, 100, 100)])
def test_partial_coverage_tiling(gpu, orc, torch, c1, tiling):
    path, soa = c1
    W, H = 640, 480
    cam = cam_for(gpu, W, H)
    t = gpu.TilingInformation(1, 1, H, W)
    t.num_tile_x, t.num_tile_y, t.width_stride, t.height_stride = tiling
    got, _ = render_gpu(gpu, torch, gpu.Scene.from_soa(soa), cam, W, H, tiling=t)
    want = orc.render(soa, cam, W, H, 3.0, tiling=tiling)
    assert_image_parity(got, want)


@pytest.mark.parametrize("W,H,k", [(1, 1, 3.0), (37, 23, 3.0), (640, 480, 0.0), (640, 480, 8.0), (17, 300, 2.0)])
def test_odd_sizes_and_k(gpu, orc, torch, c1, W, H, k):
    path, soa = c1
    cam = cam_for(gpu, W, H, fov=60)
    got, _ = render_gpu(gpu, torch, gpu.Scene.from_soa(soa), cam, W, H, k=k)
    want = orc.render(soa, cam, W, H, k)
    assert_image_parity(got, want)


def test_empty_and_all_culled(gpu, orc, torch, c1):
    path, soa = c1
    W, H = 64, 48
    cam = cam_for(gpu, W, H)
    empty = gpu.Scene.from_soa(np.zeros((38, 0), np.float32))
    got, _ = render_gpu(gpu, torch, empty, cam, W, H)
    assert not got.any()
    away = cam_for(gpu, W, H, pos=(0, 0, 4), look=(0, 0, 8))     # looking away from the cloud
    got, _ = render_gpu(gpu, torch, gpu.Scene.from_soa(soa), away, W, H)
    want = orc.render(soa, away, W, H, 3.0)
    assert not want.any()
    assert_image_parity(got, want)


def test_pair_overflow_grows_and_rerenders(gpu, orc, torch):
    """Huge splats: every one covers the whole image -> P >> the initial capacity."""
    n = 3000
    rng = np.random.default_rng(9)
    soa = np.zeros((38, n), np.float32)
    soa[0] = rng.uniform(-0.2, 0.2, n); soa[1] = rng.uniform(-0.2, 0.2, n); soa[2] = rng.uniform(-0.2, 0.2, n)
    soa[3] = rng.uniform(0.01, 0.05, n)
    soa[4:7] = rng.uniform(1.0, 2.0, (3, n))
    soa[7] = 1.0
    soa[11:38] = rng.normal(0, 0.3, (27, n))
    W, H = 640, 480
    cam = cam_for(gpu, W, H)
    r = gpu.Renderer()
    scene = gpu.Scene.from_soa(soa)
    out = torch.empty(3 * W * H, device="cuda")
    r.render(scene, cam, W, H, out.data_ptr())
    assert r.sync() == -5                      # overflow reported and buffer grown
    r.render(scene, cam, W, H, out.data_ptr())
    assert r.sync() == 0
    assert r.pair_count() > 1_000_000
    want = orc.render(soa, cam, W, H, 3.0)
    assert_image_parity(out.view(3, H, W).cpu().numpy(), want)


def test_deterministic_and_reusable_context(gpu, torch, c1):
    path, soa = c1
    W, H = 640, 480
    scene = gpu.Scene.from_soa(soa)
    r = gpu.Renderer()
    cams = [cam_for(gpu, W, H, **c) for c in CAMS]
    first = [render_gpu(gpu, torch, scene, c, W, H, renderer=r)[0] for c in cams]
    second = [render_gpu(gpu, torch, scene, c, W, H, renderer=r)[0] for c in cams]
    for a, b in zip(first, second):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_orbit_cameras_parity(gpu, orc, torch, tmp_path_factory):
    """Config-4 shape at reduced size: 8 orbit cameras (azimuth 45 deg * i)."""
    path, soa = scene_soa(gpu, tmp_path_factory, 20_000, 4)
    W, H = 480, 270
    scene = gpu.Scene.from_soa(soa)
    r = gpu.Renderer()
    for i in range(8):
        cam = cam_for(gpu, W, H)
        gpu.orbit(cam, 45.0 * i, 0.0)
        got, _ = render_gpu(gpu, torch, scene, cam, W, H, renderer=r)
        want = orc.render(soa, cam, W, H, 3.0)
        assert_image_parity(got, want)


def test_config2_full_parity(gpu, orc, torch, tmp_path_factory):
    """BASELINE config 2 at full size: 1M Gaussians, 1920x1080."""
    path, soa = scene_soa(gpu, tmp_path_factory, 1_000_000, 2)
    W, H = 1920, 1080
    cam = cam_for(gpu, W, H)
    full_size_both_blends(gpu, orc, torch, gpu.Scene.from_ply(path), soa, cam, W, H)


def test_config2_sh3_full_parity(gpu, orc, torch, tmp_path_factory):
    """BASELINE config 2 as stated — "1M random Gaussians, 1920x1080, SH degree 3" —
    through the opt-in SH-3 mode: the seed-2 PLY carries all 45 f_rest,
    Scene.from_ply(sh3=True) maps them channel-major into a 59-array block and
    k_preprocess<false, true> evaluates bands 0-3.  The reference evaluates only bands
    0-2 (render.cu:506-530; consts 369-386), so this is checked against the oracle's
    independent SH-3 restatement: colours bit-exact per visible Gaussian; for the exact
    blend the image bit-exact, for the default fast-exp blend within FX_TOL; in both
    modes the per-pixel take maps equal the oracle's and the shipped kernel's image
    equals the diagnostics build's (take_parity), so the take map describes the shipped
    composite (round-4 verdict item 6)."""
    from test_gpu_fastexp import take_parity
    path, _ = scene_soa(gpu, tmp_path_factory, 1_000_000, 2)
    W, H = 1920, 1080
    cam = cam_for(gpu, W, H)
    scene = gpu.Scene.from_ply(path, sh3=True)
    assert scene.is_sh3 and scene.n == 1_000_000
    soa3 = orc.ply_read_sh3(path)
    threads = min(16, len(os.sched_getaffinity(0)))
    with orc.sh3_mode():
        want, takes_want = orc.render_takes(soa3, cam, W, H, 3.0, threads=threads)
        want_spl = orc.preprocess(soa3, cam, W, H, 3.0)
    r = gpu.Renderer()
    linf_fast, _ = take_parity(gpu, torch, scene, cam, W, H, want, takes_want, mode=1, renderer=r)
    print(f"SH-3 config 2: fast-exp blend L-inf {linf_fast:.3g}")
    take_parity(gpu, torch, scene, cam, W, H, want, takes_want, mode=0, renderer=r)
    vis = want_spl["status"] == 2
    assert vis.sum() > 900_000
    g = r.read_splats(scene.n)[vis]
    assert np.array_equal(g["color"].view(np.uint32), want_spl["color"][vis].view(np.uint32))
    # band 3 matters: the SH-3 image is not the reference-colour image of the same file
    ref_mode = gpu.Scene.from_ply(path)
    img_ref, _ = render_gpu(gpu, torch, ref_mode, cam, W, H)
    assert not np.array_equal(img_ref, want)


def full_size_both_blends(gpu, orc, torch, scene, soa, cam, W, H):
    """The exact blend (mode 0) is bit-identical with the same take map as the oracle;
    the default fast-exp blend (mode 1) composites exactly the oracle's splats on every
    pixel (take maps, and its image equal to the diagnostics build's) within FX_TOL."""
    from test_gpu_fastexp import take_parity
    want, takes_want = orc.render_takes(soa, cam, W, H, 3.0, threads=min(16, len(os.sched_getaffinity(0))))
    take_parity(gpu, torch, scene, cam, W, H, want, takes_want, mode=0)
    linf, c = take_parity(gpu, torch, scene, cam, W, H, want, takes_want, mode=1)
    print(f"{W}x{H}: fast-exp blend L-inf {linf:.3g}, re-blended blocks {c['reblended_blocks']}")


def test_config3_full_parity_and_properties(gpu, orc, torch, tmp_path_factory):
    """BASELINE config 3 stand-in (the garden .ply cannot be fetched): 5M synthetic
    Gaussians at 1600x1063 — beyond the reference's 1,572,864-Gaussian limit
    (render.cu:904 shared-memory request)."""
    path, soa = scene_soa(gpu, tmp_path_factory, 5_000_000, 3)
    W, H = 1600, 1063
    cam = cam_for(gpu, W, H)
    scene = gpu.Scene.from_ply(path)
    got, r = render_gpu(gpu, torch, scene, cam, W, H)
    # size-independent properties: finite, in [0, 1], deterministic re-render
    assert np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= 1.0
    again, _ = render_gpu(gpu, torch, scene, cam, W, H, renderer=r)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))
    full_size_both_blends(gpu, orc, torch, scene, soa, cam, W, H)


@pytest.mark.parametrize("azimuth", [0.0, 135.0])
def test_viewer_link_binary_renders_like_oracle(gpu, orc, tmp_path, azimuth):
    """The viewer-style C++ binary (tests/link/viewer_link.cpp: reference headers,
    reference camera.cpp, by-value Camera across a real C++ call into libgsr.so, 50x50
    TilingInformation, host image) renders the oracle's image bit for bit."""
    import subprocess
    exe = os.path.join(ROOT, "oracle", "_ref", "viewer_link")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/viewer_link was not built")
    W, H = 400, 300
    ply, img = str(tmp_path / "s.ply"), str(tmp_path / "img.f32")
    gpu.write_synthetic_ply(ply, 20_000, 7)
    out = subprocess.run([exe, ply, str(W), str(H), img, str(azimuth)], capture_output=True, text=True, timeout=100)
    assert out.returncode == 0, out.stderr
    got = np.fromfile(img, dtype=np.float32).reshape(3, H, W)
    cam = cam_for(gpu, W, H)
    if azimuth:
        gpu.orbit(cam, azimuth, 0.0)
    t = gpu.TilingInformation(50, 50, H, W)
    want = orc.render(gpu.read_ply(ply), cam, W, H, 3.0, tiling=(t.num_tile_x, t.num_tile_y, t.width_stride,
                                                                     t.height_stride))
    assert (want != 0).sum() > 1000
    assert_image_parity(got, want)
