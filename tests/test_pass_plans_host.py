"""CPU tests of the launch plans of the event-time and the resampling pass: kin::event_plan (event_kernels.hip) and
kin::resample_plan (resample_kernels.hip), pure host functions of the product library, called through
tests/native/pass_plan_host.cpp. The rules are restated here from the comments of the two launchers; the GPU tests
(test_gpu_event_times.py, test_gpu_resample.py) run the kernels under every plan these rules can give."""
import pytest

from tests import res_host

N_CUS = (256, 1)
KNOBS = ("KIN_EVENT_WAVES", "KIN_EVENT_PART_ROWS", "KIN_RESAMPLE_TILE_QUERIES", "KIN_RESAMPLE_WAVES")
IGNORED = ("0", "-1", "x", "")


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)


def ceil_div(a, b):
    return -(-a // b)


def test_constants_are_those_the_cases_are_built_for():
    import event_cases as ec
    import resample_cases as rc
    c = res_host.plan_constants()
    assert c == dict(EVENT_LANES=ec.LANES, EVENT_WAVES_MAX=16, EVENT_ROWS_IN_FLIGHT=ec.ROWS_IN_FLIGHT, RESAMPLE_SLICE=rc.SLICE,
                     RESAMPLE_WAVES_MAX=16, RESAMPLE_TILE_MAX=256)
    assert ec.PART_ROWS == c["EVENT_ROWS_IN_FLIGHT"]       # (why the knob matrix adds parts of 1, 3, 5 and 6 rows)
    assert max(t for t, _ in rc.PLANS) == c["RESAMPLE_TILE_MAX"] and max(w for _, w in rc.PLANS) == c["RESAMPLE_WAVES_MAX"]
    # the restated plan of event_cases.py is the launcher's
    for L in (1, 9, 17, 37):
        assert ec.knob_plan({}, L) == res_host.event_plan(2, L, 130, 256)


@pytest.mark.parametrize("n_cu", N_CUS + (0,))
def test_event_plan_chooses_4_8_or_16_wavefronts_at_the_two_thresholds(n_cu):
    """groups = S ceil(N / 64) workgroups; four wavefronts each when 4 groups >= 8 n_cu, eight when 8 groups >= 8 n_cu, else 16."""
    want = 8 * max(n_cu, 1)
    for at in (want // 4, want // 8):
        for groups in (at - 1, at, at + 1):
            expect = 4 if groups * 4 >= want else 8 if groups * 8 >= want else 16
            assert res_host.event_plan(groups, 100, 64, n_cu)[0] == expect, (groups, n_cu)          # groups segments of one group
            assert res_host.event_plan(groups, 100, 1, n_cu)[0] == expect, (groups, n_cu)
            if groups >= 1:                                                                       # one segment of `groups` groups
                for N in (64 * groups, 64 * (groups - 1) + 1):
                    assert res_host.event_plan(1, 100, N, n_cu)[0] == expect, (N, n_cu)
    assert {res_host.event_plan(g, 100, 64, n_cu)[0] for g in (want // 4, want // 8, want // 8 - 1)} == {4, 8, 16}


def test_event_waves_knob_is_honoured_from_1_to_16_and_ignored_outside(monkeypatch):
    for S in (1, 300, 5000):
        own = res_host.event_plan(S, 100, 64, 256)[0]
        for v in range(1, 17):
            monkeypatch.setenv("KIN_EVENT_WAVES", str(v))
            assert res_host.event_plan(S, 100, 64, 256)[0] == v
        for v in IGNORED + ("17", "64", "4294967297"):
            monkeypatch.setenv("KIN_EVENT_WAVES", v)
            assert res_host.event_plan(S, 100, 64, 256)[0] == own, v
    monkeypatch.delenv("KIN_EVENT_WAVES")
    assert [res_host.event_plan(S, 100, 64, 256)[0] for S in (1, 300, 5000)] == [16, 8, 4]


LENGTHS = (0, 1, 4, 5, 63, 64, 65, 10_000, 2 ** 31 - 1)


@pytest.mark.parametrize("n_cu", N_CUS)
def test_event_part_rows_cover_the_segment_in_multiples_of_the_rows_in_flight(n_cu, monkeypatch):
    F = res_host.plan_constants()["EVENT_ROWS_IN_FLIGHT"]
    want = 8 * n_cu
    for L in LENGTHS:
        for S in (1, want // 8, want // 4):                  # the launcher's own 16, 8 and 4 wavefronts
            waves, rows = res_host.event_plan(S, L, 64, n_cu)
            assert rows % F == 0 and rows >= F and waves * rows >= L, (L, S)
            assert rows == max(F, ceil_div(ceil_div(max(L, 1), waves), F) * F)          # no larger than it has to be
            # KIN_EVENT_PART_ROWS only lowers it
            for v in (1, 3, F, F + 1, rows - 1, rows, rows + 1, 2 ** 40):
                if v >= 1:
                    monkeypatch.setenv("KIN_EVENT_PART_ROWS", str(v))
                    assert res_host.event_plan(S, L, 64, n_cu) == (waves, min(rows, v)), (L, S, v)
            for v in IGNORED:
                monkeypatch.setenv("KIN_EVENT_PART_ROWS", v)
                assert res_host.event_plan(S, L, 64, n_cu) == (waves, rows), (L, S, v)
            monkeypatch.delenv("KIN_EVENT_PART_ROWS")
        # a forced wavefront count: the same rule; one wavefront over 2^31 - 1 rows gets one part of all of them (the largest int)
        for forced in range(1, 17):
            monkeypatch.setenv("KIN_EVENT_WAVES", str(forced))
            waves, rows = res_host.event_plan(1, L, 64, n_cu)
            assert waves == forced and rows >= F and waves * rows >= L, (L, forced)
            assert rows == min(max(F, ceil_div(ceil_div(max(L, 1), forced), F) * F), 2 ** 31 - 1), (L, forced)
        monkeypatch.delenv("KIN_EVENT_WAVES")


def _tile(S, Q, N, n_cu):
    """The largest tile of 32, 16, 8 with which the grid has two workgroups per compute unit, else 4."""
    slices = ceil_div(max(N, 1), 1024)
    for tile in (32, 16, 8):
        if S * ceil_div(max(Q, 1), tile) * slices >= 2 * max(n_cu, 1):
            return tile
    return 4


def test_resample_plan_table():
    table = {
        (256, 9, 300, 256): 8, (1, 9, 300, 256): 4, (4096, 64, 300, 256): 32,
        (128, 9, 1024, 256): 4, (128, 9, 1025, 256): 8,          # a second species slice doubles the grid
        (256, 9, 1025, 256): 32, (32, 64, 1025, 256): 8, (32, 64, 2049, 256): 8, (32, 64, 3073, 256): 16,
        (1, 9, 300, 1): 8, (1, 1, 1, 1): 4, (2, 1, 1, 1): 32, (1, 33, 1, 1): 32, (1, 32, 1, 1): 16, (1, 1, 1025, 1): 32,
    }
    for (S, Q, N, n_cu), tile in table.items():
        assert _tile(S, Q, N, n_cu) == tile, (S, Q, N, n_cu)                       # (the restated rule gives the table)
        assert res_host.resample_plan(S, Q, N, n_cu) == (tile, 4), (S, Q, N, n_cu)
    seen = set()
    for n_cu in N_CUS + (0,):
        for S in (0, 1, 2, 3, 31, 32, 33, 64, 127, 128, 129, 255, 256, 257, 511, 512, 513, 4096):
            for Q in (0, 1, 8, 9, 16, 17, 32, 33, 70, 450):
                for N in (1, 1024, 1025, 2048, 2049):
                    tile, waves = res_host.resample_plan(S, Q, N, n_cu)
                    assert tile in (4, 8, 16, 32) and waves == 4 and tile == _tile(S, Q, N, n_cu), (S, Q, N, n_cu)
                    seen.add(tile)
    assert seen == {4, 8, 16, 32}


def test_resample_knobs_are_honoured_in_their_ranges_and_ignored_outside(monkeypatch):
    own = res_host.resample_plan(256, 9, 300, 256)
    assert own == (8, 4)
    for v in (1, 2, 3, 4, 5, 31, 33, 255, 256):
        monkeypatch.setenv("KIN_RESAMPLE_TILE_QUERIES", str(v))
        assert res_host.resample_plan(256, 9, 300, 256) == (v, 4)
    for v in IGNORED + ("257", "4294967297"):
        monkeypatch.setenv("KIN_RESAMPLE_TILE_QUERIES", v)
        assert res_host.resample_plan(256, 9, 300, 256) == own, v
    monkeypatch.delenv("KIN_RESAMPLE_TILE_QUERIES")
    for v in range(1, 17):
        monkeypatch.setenv("KIN_RESAMPLE_WAVES", str(v))
        assert res_host.resample_plan(256, 9, 300, 256) == (8, v)
    for v in IGNORED + ("17", "4294967297"):
        monkeypatch.setenv("KIN_RESAMPLE_WAVES", v)
        assert res_host.resample_plan(256, 9, 300, 256) == own, v
    monkeypatch.setenv("KIN_RESAMPLE_TILE_QUERIES", "256")
    monkeypatch.setenv("KIN_RESAMPLE_WAVES", "1")
    assert res_host.resample_plan(3, 70, 65, 256) == (256, 1)          # the tile larger than its workgroup
