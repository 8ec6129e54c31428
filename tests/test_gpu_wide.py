"""The culls, spans and blends on large, tilted and clipped splats (tests/_wide_scenes.py).

Every conservative shortcut of the forward path proves "this pair, block or pixel cannot
composite": the tile row spans, the blend's ellipse-vs-block test, the cull word's fast-path
proof, the fast-exp guard, the saturation filter.  The synthetic .ply's splats are about 7
pixels across and the hand-made dense scenes carry the identity quaternion; the scenes here
have tile rects wider than six tiles and taller than four rows, tilted needles whose edge
crosses many 8x8 blocks, centres up to 15,000 pixels off screen, boxes that end at W and H,
conics on both sides of the robust-PD test, pixels that saturate early and pixels that never
do (tests/test_wide_scenes.py asserts all that on the oracle's records).  The comparisons are
the suite's own (test_gpu_parity, test_gpu_fastexp, test_gpu_depth_split,
test_gpu_path_shared), against the unmodified oracle, at 320x240 unless stated."""
import os

import numpy as np
import pytest

import _wide_scenes as ws
from conftest import exact_blend
from test_gpu_depth_split import KNOB_UNSAT, check_takes, split_renderer
from test_gpu_fastexp import take_parity
from test_gpu_parity import (BINNING_KNOBS, CAMS, KNOB_TILE_SPANS, assert_image_parity, cam_for,
                             check_binning_matches_pair_sort, check_preprocess_records, check_tile_spans, render_gpu)
from test_gpu_path_shared import LAUNCHES, path_images, renderer as path_renderer

pytestmark = pytest.mark.gpu

W, H = ws.W, ws.H
ORC_THREADS = min(16, len(os.sched_getaffinity(0)))
GRAZE = [f"graze{s}" for s in ws.GRAZE_SEEDS]


@pytest.fixture(scope="module")
def torch(gpu):
    import torch as t
    assert t.cuda.is_available()
    return t


_soa, _want = {}, {}


def soa_of(name):
    if name not in _soa:
        _soa[name] = ws.graze(int(name[5:])) if name.startswith("graze") else ws.scene(name)
        _soa[name].setflags(write=False)
    return _soa[name]


def oracle_frame(orc, gpu, name, ci, W=W, H=H, k=3.0, tiling=None):
    """(camera, image, take map) of one case from the oracle, computed once and left unchanged."""
    key = (name, ci, W, H, k, tiling)
    if key not in _want:
        cam = cam_for(gpu, W, H, **CAMS[ci])
        img, takes = orc.render_takes(soa_of(name), cam, W, H, k, tiling=tiling, threads=ORC_THREADS)
        img.setflags(write=False), takes.setflags(write=False)
        _want[key] = (cam, img, takes)
    return _want[key]


# ---------------------------------------------------------------- a. records, order, lists

@pytest.mark.parametrize("name,ci", [(s, ci) for s in ("slabs", "needles", "huge") for ci in range(len(CAMS))]
                         + [(g, 0) for g in GRAZE])
def test_preprocess_records_bit_exact(gpu, orc, name, ci):
    """test_gpu_parity's record test: px_x / px_y thousands of pixels off screen, ranges equal
    to W / H, rects across the whole grid; depth order, tile_count, pair list and tile ranges."""
    want = check_preprocess_records(gpu, orc, soa_of(name), cam_for(gpu, W, H, **CAMS[ci]), W, H,
                                    pairs_of=ws.rect_pairs)
    v = want[want["status"] == 2]
    assert (v["aabb"][:, 2] == W).any() and (v["aabb"][:, 3] == H).any()
    if name.startswith("graze"):
        assert max(np.abs(v["px_x"]).max(), np.abs(v["px_y"]).max()) > 8192


# ---------------------------------------------------------------- b. spans drop only unreachable pairs

# (scene, camera, k, floor of the dropped share).  The floor keeps spans that were switched
# off from passing: 0.10 on slabs and needles, whose splats are small against their 3- or
# 8-sigma boxes (the numpy model of tools/sim/spans_check.py predicts 0.13 - 0.27), above 0
# where most rects are clipped by the frame (stack, huge, graze: 0.01 - 0.07) and at k = 1,
# where the box is the 1-sigma one and lies inside the alpha >= 1e-3 ellipse of every splat
# whose opacity is above 1e-3 e (the model: 0.08).
SPAN_CASES = ([("slabs", ci, 3.0, 0.10) for ci in range(4)] + [("slabs", ci, 8.0, 0.10) for ci in (0, 2)]
              + [("slabs", ci, 1.0, 0.0) for ci in (0, 2)] + [("needles", ci, 3.0, 0.10) for ci in range(4)]
              + [(s, ci, 3.0, 0.0) for s in ("stack", "huge") for ci in range(4)] + [(g, 0, 3.0, 0.0) for g in GRAZE])


@pytest.mark.parametrize("name,ci,k,floor", SPAN_CASES)
def test_tile_spans_drop_only_unreachable_pairs(gpu, orc, torch, name, ci, k, floor):
    """test_gpu_parity's spans test: the spans-on list is a subsequence of the full one, every
    dropped pair stays below the blend's own alpha threshold of 1e-3 on its tile, exact images
    are bit-identical with spans on and off and equal the oracle's."""
    full, dropped, peak = check_tile_spans(gpu, orc, torch, soa_of(name), cam_for(gpu, W, H, **CAMS[ci]), W, H, k=k,
                                           floor=0.0, pairs_of=ws.rect_pairs)
    print(f"{name} camera {ci} k {k:g}: dropped share {dropped / full:.4f}, largest dropped alpha {peak:.4e}")
    assert dropped > 0 and dropped >= floor * full


# ---------------------------------------------------------------- c. both blends, take maps

@pytest.mark.parametrize("name,ci", [(s, ci) for s in ("slabs", "needles", "stack", "graze0") for ci in (0, 2)]
                         + [(g, 0) for g in GRAZE[1:]])
def test_take_maps_both_blends(gpu, orc, torch, name, ci):
    """The exact blend is bit-exact and re-blends nothing; the fast blend composites exactly
    the oracle's splats on every pixel, within FX_TOL.  (Camera 2 looks past every splat of
    graze: a frame in which all are culled.)"""
    cam, want, takes = oracle_frame(orc, gpu, name, ci)
    scene = gpu.Scene.from_soa(soa_of(name))
    if (name, ci) != ("graze0", 2):
        assert (takes & np.uint64(0xFFFFFFFF)).max() > 3
    linf, ce = take_parity(gpu, torch, scene, cam, W, H, want, takes, mode=0)
    assert linf == 0.0 and ce["reblended_blocks"] == 0
    linf, cf = take_parity(gpu, torch, scene, cam, W, H, want, takes, mode=1)
    print(f"{name} camera {ci}: fast-exp blend L-inf {linf:.3g}, re-blended blocks {cf['reblended_blocks']}, "
          f"slow-path iterations {ce['slow_path_iters']} exact / {cf['slow_path_iters']} fast")
    if name == "needles":       # records without the fast-path proof ran the one-splat path
        assert ce["slow_path_iters"] > 0 and cf["slow_path_iters"] > 0


@pytest.mark.parametrize("name,ci", [("slabs", 0), ("slabs", 2), ("stack", 0), ("stack", 1), ("stack", 2)])
def test_fast_blend_runs_on_wide_splats(gpu, orc, torch, name, ci):
    """The scenes with opacity capped at 1 (_wide_scenes.unit_opacity), so that the fast blend
    itself composites them and does not hand the block to the exact blend: the oracle's take
    maps, colours within FX_TOL.  Every record of these two scenes is robustly positive
    definite, so a block is blended again only where a pixel's transmittance passes within the
    guard band (1.2e-4 relative) of 1e-3: a few per cent of the blocks of stack, none of slabs,
    where no pixel saturates.  A quarter of the blocks is the floor under which the fast path
    counts as having run."""
    soa = ws.unit_opacity(soa_of(name))
    assert (soa_of(name)[3] > 1).sum() >= 10 and (soa[3] == 1).sum() >= 10
    cam = cam_for(gpu, W, H, **CAMS[ci])
    want, takes = orc.render_takes(soa, cam, W, H, 3.0, threads=ORC_THREADS)
    assert (takes & np.uint64(0xFFFFFFFF)).max() > 3
    linf, c = take_parity(gpu, torch, gpu.Scene.from_soa(soa), cam, W, H, want, takes, mode=1)
    nblocks = 4 * ((W + 15) // 16) * ((H + 15) // 16)
    print(f"{name} camera {ci}, opacity <= 1: fast-exp blend L-inf {linf:.3g}, re-blended blocks "
          f"{c['reblended_blocks']} of {nblocks}, suspect pixels {c['suspect_pixels']}")
    assert c["reblended_blocks"] <= nblocks // 4


# ---------------------------------------------------------------- d. binning paths

@pytest.mark.parametrize("knobs", BINNING_KNOBS)
@pytest.mark.parametrize("name,ci", [("slabs", 2), ("stack", 1)])
def test_tile_binning_matches_pair_sort(gpu, orc, torch, name, ci, knobs):
    """One splat expands into hundreds of (tile row, column) items: binning equals the pair
    sort in pairs, order and image, and equals the oracle."""
    check_binning_matches_pair_sort(gpu, orc, torch, soa_of(name), cam_for(gpu, W, H, **CAMS[ci]), W, H, knobs)


def test_tile_binning_8bit_digits_wide_rects(gpu, orc, torch):
    """2100 x 2060 (132 x 129 tiles) over 48 slabs with scales of 0.05 - 1.5: rects wider than
    128 tile columns and taller than 128 tile rows, so one splat's items carry digits above
    127 in both binning scatters.  Spans on and off against the pair sort and the oracle."""
    Wb, Hb = 2100, 2060
    soa = ws.scene("slabs", n=48, scales=(0.05, 1.5))
    cam = cam_for(gpu, Wb, Hb, **CAMS[0])
    x0, x1, y0, y1 = ws.tile_rects(orc.preprocess(soa, cam, Wb, Hb, 3.0), Wb, Hb)
    assert (x1 - x0 + 1 > 128).any() and (y1 - y0 + 1 > 128).any()
    scene = gpu.Scene.from_soa(soa)
    r_bin, r_sort, r_span = (exact_blend(gpu.Renderer()) for _ in range(3))
    r_bin.set_tuning(KNOB_TILE_SPANS, 0)
    r_sort.set_tuning(7, 0)                 # (the pair sort lists every tile of every rect)
    r_span.set_tuning(KNOB_TILE_SPANS, 1)
    imgs = [render_gpu(gpu, torch, scene, cam, Wb, Hb, renderer=r)[0] for r in (r_bin, r_sort, r_span)]
    tx, ty = r_bin.tile_grid()
    assert tx > 128 and ty > 128 and r_bin.row_item_count() > 0 and r_sort.row_item_count() == -1
    full, spanned = r_bin.read_pairs(), r_span.read_pairs()
    assert full.size > 100_000
    assert np.array_equal(full, r_sort.read_pairs())
    assert 0 < spanned.size < full.size
    assert np.array_equal(spanned, full[np.isin(full, spanned)])     # a subsequence of the full list
    want = orc.render(soa, cam, Wb, Hb, 3.0, threads=ORC_THREADS)
    for img in imgs:
        assert_image_parity(img, want, exact=True)


# ---------------------------------------------------------------- e. odd frame, partial tiling

@pytest.mark.parametrize("Wo,Ho,tiling", [(333, 217, (4, 3, 70, 50)), (37, 23, None), (1, 1, None)])
def test_odd_frames_and_partial_tiling(gpu, orc, torch, Wo, Ho, tiling):
    """slabs where the frame cuts tiles and blocks, and where a tiling covers 280 x 150 of
    333 x 217 (pixels outside stay 0): exact, the oracle's take maps, in both blends."""
    cam, want, takes = oracle_frame(orc, gpu, "slabs", 2, Wo, Ho, tiling=tiling)
    t = None
    if tiling:
        t = gpu.TilingInformation(1, 1, Ho, Wo)
        t.num_tile_x, t.num_tile_y, t.width_stride, t.height_stride = tiling
        assert not want[:, 150:, :].any() and not want[:, :, 280:].any()
    assert (takes & np.uint64(0xFFFFFFFF)).max() > 3
    scene = gpu.Scene.from_soa(soa_of("slabs"))
    linf, c = take_parity(gpu, torch, scene, cam, Wo, Ho, want, takes, mode=0, tiling=t)
    assert linf == 0.0 and c["reblended_blocks"] == 0
    take_parity(gpu, torch, scene, cam, Wo, Ho, want, takes, mode=1, tiling=t)


# ---------------------------------------------------------------- f. shared preprocess

@pytest.mark.parametrize("exact", [True, False])
def test_shared_preprocess_equals_per_frame_and_oracle(gpu, orc, torch, exact):
    """gsr_render_path, four frames in flight over the four cameras of slabs: one
    k_preprocess_multi launch writes all four lanes' records.  Each frame equals the
    per-frame path's and a plain render's bit for bit, and the oracle's by its blend's rule."""
    scene = gpu.Scene.from_soa(soa_of("slabs"))
    cams = [cam_for(gpu, W, H, **c) for c in CAMS]
    on, off = path_renderer(gpu, 4, True, exact), path_renderer(gpu, 4, False, exact)
    a = path_images(gpu, torch, on, scene, cams)
    b = path_images(gpu, torch, off, scene, cams)
    assert on.get_tuning(LAUNCHES) > 0 and off.get_tuning(LAUNCHES) == 0
    for ci, cam in enumerate(cams):
        r = gpu.Renderer()
        r.set_tuning(22, 0 if exact else 1)
        single, _ = render_gpu(gpu, torch, scene, cam, W, H, renderer=r)
        assert np.array_equal(a[ci].view(np.uint32), b[ci].view(np.uint32)), f"frame {ci}: shared vs per-frame path"
        assert np.array_equal(a[ci].view(np.uint32), single.view(np.uint32)), f"frame {ci}: shared vs plain render"
        assert_image_parity(a[ci], oracle_frame(orc, gpu, "slabs", ci)[1], exact=exact)


# ---------------------------------------------------------------- g. forced depth split

@pytest.mark.parametrize("pm", [50, 500])
@pytest.mark.parametrize("ci", [0, 1])
def test_forced_depth_split(gpu, orc, torch, ci, pm):
    """stack with the split forced at 5 % and 50 % of the depth order: every splat spans many
    tiles, so phase A's lists are long and phase B resumes blocks that phase A left
    unsaturated (camera 1: 8 % of the pixels never saturate).  Exact, the oracle's take maps."""
    cam, want, takes = oracle_frame(orc, gpu, "stack", ci)
    scene = gpu.Scene.from_soa(soa_of("stack"))
    r = split_renderer(gpu, 1, pm)
    img, _ = render_gpu(gpu, torch, scene, cam, W, H, renderer=r)
    unsat = r.get_tuning(KNOB_UNSAT)
    print(f"stack camera {ci}, split at {pm / 10:g} %: blocks left to phase B {unsat}")
    if ci == 1:
        assert unsat > 0
    assert_image_parity(img, want, exact=True)
    r.set_tuning(24, pm)
    check_takes(gpu, torch, r, scene, cam, W, H, want, takes)
    r.close()
