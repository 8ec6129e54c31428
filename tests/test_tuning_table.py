"""Every tuning knob of include/gsr.h (gsr_get_tuning / gsr_set_tuning): its default, every
value it accepts or refuses out of one candidate set, what a boolean knob reads back, that a
refused value leaves the earlier one in place, and the text gsr_last_error then holds.  Host
code only: a context exists without a device, so this needs no GPU."""
import pytest

CANDIDATES = (-1, 0, 1, 2, 3, 4, 5, 8, 16, 17, 999, 1000, 1024, 2048, 4096, 8192, 8193, 65536, 65537, 1 << 20)
ITEMS = "binning items per thread must be 4, 8 or 16"

# knob: (default, accepted candidates, refusal text)
SETTABLE = {
    0: (0, {0, 3}, "blend schedule must be 0 (default) or 3 (timeline stamps)"),
    1: (16, {8, 16}, "tile-sort items must be 8 or 16"),
    2: (0, {0, 4, 8, 16}, "depth-sort items must be 0, 4, 8 or 16"),
    3: (1024, range(0, 8193), "bad group cap"),
    4: (0, range(0, 8193), "bad group cap"),
    8: (4, {4, 8, 16}, ITEMS),
    9: (8, {4, 8, 16}, ITEMS),
    10: (0, range(0, 65537), "bad column-pass group count"),
    13: (4, range(0, 65537), "blend band tiles must be 0..65536"),
    18: (2, {0, 1, 2}, "depth compaction must be 0, 1 or 2"),
    19: (2, {0, 1, 2}, "tile spans must be 0, 1 or 2"),
    20: (1, {0, 1}, "rank path must be 0 or 1"),
    22: (1, {0, 1, 2}, "blend exp must be 0, 1 or 2"),
    23: (2, {0, 1, 2}, "depth split must be 0, 1 or 2"),
    24: (250, range(1, 1000), "split point must be 1..999"),
    28: (1, range(0, 4), "depth buckets must be 0..3"),
    31: (0, {0, 1024, 2048}, "column chunk must be 0, 1024 or 2048"),
    32: (0, range(0, (1 << 20) + 1), "fail frame must be >= 0"),
    34: (1, {0, 1}, "shared preprocess must be 0 or 1"),
}
BOOLEAN = (5, 6, 7, 11, 30)          # default 1; stored as value != 0
READ_ONLY = (21, 25, 26, 29, 33, 35)
UNKNOWN = (12, 14, 15, 16, 17, 27, 36, 37, -1)
GSR_E_ARG = -1                       # include/gsr.h


@pytest.fixture
def renderer(gsr, monkeypatch):
    """A fresh renderer per test case, with the two environment defaults cleared."""
    monkeypatch.delenv("GSR_RANK_ATOMIC", raising=False)
    monkeypatch.delenv("GSR_BLEND_EXP", raising=False)
    r = gsr.Renderer()
    yield r
    r.close()


def test_the_table_covers_every_knob():
    assert sorted([*SETTABLE, *BOOLEAN, *READ_ONLY, *(k for k in UNKNOWN if k >= 0)]) == list(range(38))


@pytest.mark.parametrize("knob", sorted(SETTABLE))
def test_settable_knob(gsr, renderer, knob):
    default, accepted, text = SETTABLE[knob]
    assert renderer.get_tuning(knob) == default
    current = default
    assert any(v in accepted for v in CANDIDATES) and any(v not in accepted for v in CANDIDATES)
    for v in CANDIDATES:
        if v in accepted:
            renderer.set_tuning(knob, v)
            current = v
        else:
            with pytest.raises(gsr.GsrError) as err:
                renderer.set_tuning(knob, v)
            assert err.value.code == GSR_E_ARG
            assert f"gsr_set_tuning: {text}" in str(err.value), (knob, v)
        assert renderer.get_tuning(knob) == current, (knob, v)   # a refused value changes nothing


@pytest.mark.parametrize("knob", BOOLEAN)
def test_boolean_knob(renderer, knob):
    assert renderer.get_tuning(knob) == 1
    for v in CANDIDATES + (0, -1):
        renderer.set_tuning(knob, v)   # any value is accepted
        assert renderer.get_tuning(knob) == (0 if v == 0 else 1), (knob, v)


@pytest.mark.parametrize("knob", READ_ONLY)
def test_read_only_knob(gsr, renderer, knob):
    if knob != 21:   # GSR_TUNE_RANK_ATOMIC_ACTIVE's read asks the device
        assert renderer.get_tuning(knob) == 0
    for v in CANDIDATES:
        with pytest.raises(gsr.GsrError) as err:
            renderer.set_tuning(knob, v)
        assert err.value.code == GSR_E_ARG
        assert f"gsr_set_tuning: knob {knob} is read-only" in str(err.value)
    if knob != 21:
        assert renderer.get_tuning(knob) == 0


@pytest.mark.parametrize("knob", UNKNOWN)
def test_unknown_knob(gsr, renderer, knob):
    with pytest.raises(gsr.GsrError) as err:
        renderer.get_tuning(knob)
    assert err.value.code == GSR_E_ARG and "gsr_get_tuning: unknown knob" in str(err.value)
    for v in CANDIDATES:
        with pytest.raises(gsr.GsrError) as err:
            renderer.set_tuning(knob, v)
        assert err.value.code == GSR_E_ARG and "gsr_set_tuning: unknown knob" in str(err.value)


def test_environment_defaults(gsr, monkeypatch):
    """GSR_RANK_ATOMIC is read when the knob is (until a frame or a set fixes it), GSR_BLEND_EXP
    when the context is created."""
    monkeypatch.delenv("GSR_RANK_ATOMIC", raising=False)
    monkeypatch.setenv("GSR_BLEND_EXP", "0")
    r = gsr.Renderer()
    monkeypatch.delenv("GSR_BLEND_EXP")
    try:
        assert r.get_tuning(22) == 0
        assert r.get_tuning(20) == 1
        monkeypatch.setenv("GSR_RANK_ATOMIC", "0")
        assert r.get_tuning(20) == 0
        r.set_tuning(20, 1)
        assert r.get_tuning(20) == 1
    finally:
        r.close()
    r = gsr.Renderer()
    try:
        assert r.get_tuning(22) == 1   # the environment no longer says otherwise
    finally:
        r.close()
