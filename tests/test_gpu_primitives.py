"""The device primitives at their edges, one by one: mathfn.h, wave_ops.h, philox.h and the searches, the collision tests and
the pieces of the one-launch waypoint index (lb_scan, lb_reach, lb_tag, lb_publish / lb_wait) of mppi_device.h, through the
test-only harness tests/device/prims_harness.hip (libmppi_prims.so, the product's compiler flags).
Inputs, f64 references and comparisons live in tests/prims_checks.py; tools/prims_report.py prints the figures these tests
bound (profiles/prims_measured.json).  The search kernels only store the index a search returns, so a wrong index is a
failed assertion here and never an address.  The look-back exchange runs B one-wave workgroups whose waits end by their own
clock and return a status: a word that never arrives is a result (ok = 0), not a hang."""
import numpy as np
import pytest

import prims_checks as pc
from oracle import philox
from prims_checks import F32, F64, I32, U32

pytestmark = pytest.mark.gpu

FP = [pytest.param(F32, id="f32"), pytest.param(F64, id="f64")]


@pytest.fixture(scope="module")
def P():
    import dnn_mppi_mpc_amd as pkg
    return pc.Prims(pkg.build.prims_library())


# ------------------------------------------------------------------------------------------ mathfn (f32 overloads)
def test_sincos_polynomial_branch_within_2_ulp_and_library_branch(P):
    e = pc.sincos_errors(P)
    print("sincos_", e)
    assert e["sin_ulp"] <= 2.0 and e["cos_ulp"] <= 2.0, e  # mathfn.h: "<= 2 ulp for |x| < 2^15"
    assert e["library_abs"] <= 2.0 ** -22, e  # any correct large-argument reduction; a wrong one is off by ~1


def test_tan_within_2_ulp_and_continuous_across_the_branch(P):
    e = pc.tan_errors(P)
    print("tan_", e)
    assert e["tan_ulp"] <= 2.0, e  # mathfn.h: "<= 2 ulp there"
    assert e["tan_outside_ulp"] <= 2.0, e  # the first arguments that take tanf


def test_pymod_stays_in_range_and_on_the_circle(P):
    r, a, circ = pc.pymod_check(P)
    print("pymod max circular error", circ.max(), "at", a[circ.argmax()])
    bad = ~((r >= 0) & (r < pc.PYMOD_M))  # the invariant the yaw wrap relies on: [0, m) strictly (NaN fails too)
    assert not bad.any(), (a[bad][:8], r[bad][:8])
    assert circ.max() <= 2.0 ** -21, (circ.max(), a[circ.argmax()])  # 1 ulp at m


def test_exp_weight_of_the_minimum_is_one_and_the_tail_is_finite(P):
    one = P.exp(np.array([0.0, -0.0], F32))
    assert (one == F32(1.0)).all(), one  # the minimum-cost sample weighs exactly 1
    rel, bound = pc.exp_rel_err(P)
    print("exp_ max relative error", rel.max(), "max error / bound", (rel / bound).max())
    assert (rel <= bound).all(), (rel / bound).max()
    small = P.exp(np.array([-1e-8], F32))
    assert abs(float(small[0]) - np.exp(-1e-8)) <= 4 * 2.0 ** -24
    tail = P.exp(np.array([-87.4, -100.0, -1e4, -np.inf], F32))
    assert np.isfinite(tail).all() and (tail >= 0).all() and (tail <= 2.0 ** -126).all(), tail
    assert tail[-1] == 0.0


@pytest.mark.parametrize("dtype", FP)
def test_clamp_equals_np_clip(P, dtype):
    # (no NaN: v_med3_f32 and the generic template differ there, and a NaN control is outside the contract)
    lim = dtype(3.14) if dtype == F32 else dtype(0.523)
    rng = np.random.default_rng(15)
    inf = dtype(np.inf)
    edge = [0.0, -0.0, lim, -lim, np.nextafter(lim, inf), np.nextafter(lim, -inf), np.nextafter(-lim, inf),
            np.nextafter(-lim, -inf), np.inf, -np.inf, 1e-40 if dtype == F32 else 5e-324]
    v = np.concatenate([np.array(edge, dtype), rng.normal(0, 2 * float(lim), 4096).astype(dtype)])
    got = P.clamp(v, float(lim), dtype)
    assert np.array_equal(got, np.clip(v, -lim, lim))


# ------------------------------------------------------------------------------------------ wave_ops
SCAN_CASES = [(F32, 0, "add"), (F32, 1, "min"), (F64, 0, "add"), (F64, 1, "min"), (I32, 0, "min"), (I32, 1, "max")]


@pytest.mark.parametrize("dtype,op,name", SCAN_CASES, ids=[f"{pc._sfx(d)}-{n}" for d, _, n in SCAN_CASES])
@pytest.mark.parametrize("variant", [pc.SCAN, pc.HALF, pc.ROW, pc.SEG1, pc.SEG2, pc.REDUCE],
                         ids=["scan_incl", "scan_incl_half", "scan_incl_row", "seg1", "seg2", "reduce"])
def test_scans_bitwise(P, variant, dtype, op, name):
    for seed in (41, 42, 43):
        x = pc.scan_input(dtype, name, seed)
        got, want = P.scan(op, variant, x), pc.scan_reference(name, variant, x)
        assert np.array_equal(pc.bits(got), pc.bits(want)), (seed, np.nonzero(pc.bits(got) != pc.bits(want))[0])


@pytest.mark.parametrize("dtype", FP)
def test_shifts_carry_into_lane_0_and_lane_32(P, dtype):
    x = np.random.default_rng(44).normal(size=64).astype(dtype)
    carry = dtype(-7.25)
    whole = np.concatenate([[carry], x[:-1]]).astype(dtype)
    half = whole.copy()
    half[32] = carry
    for variant, want in ((0, whole), (1, half), (2, whole), (3, half)):
        assert np.array_equal(pc.bits(P.shift(variant, x, float(carry))), pc.bits(want)), variant


@pytest.mark.parametrize("dtype", FP)
def test_read_lane_and_shfl_xor(P, dtype):
    x = np.random.default_rng(45).normal(size=64).astype(dtype)  # (f64: both halves of every value carry information)
    got = P.read_lane(x)
    assert np.array_equal(pc.bits(got), pc.bits(np.repeat(x[:, None], 64, axis=1)))
    for m in (1, 2, 4, 8, 16, 32):
        assert np.array_equal(pc.bits(P.shfl_xor(m, x)), pc.bits(x[np.arange(64) ^ m])), m


@pytest.mark.parametrize("dtype", FP)
def test_argmin_first_is_the_first_minimum_on_every_lane(P, dtype):
    rng = np.random.default_rng(46)
    lane = np.arange(64)

    def check(d, j, want_d, want_j, tag):
        do, jo = P.argmin_first(d.astype(dtype), j)
        assert (jo == want_j).all() and (do == dtype(want_d)).all(), (tag, jo, do)

    for at in (0, 15, 16, 31, 32, 47, 48, 63):  # a unique minimum in every row's first and last lane
        d = rng.uniform(1.0, 2.0, 64)
        d[at] = 0.5
        check(d, 3 * lane + 1, 0.5, 3 * at + 1, at)
    d = rng.uniform(1.0, 2.0, 64)
    d[[5, 37]] = 0.25
    check(d, 63 - lane, 0.25, 63 - 37, "tie: the smaller j sits on the higher lane")
    check(np.full(64, 1.5), 63 - lane, 1.5, 0, "all equal")
    check(np.full(64, np.inf), lane + 1, np.inf, 1, "all +inf")


@pytest.mark.parametrize("dtype", FP)
def test_argmin_first_without_a_candidate_returns_zero(P, dtype):
    """No lane holds a candidate that compared smaller (the searches start from j = INT_MAX), or the distances are NaN: the
    offset is 0, the first candidate, as np.argmin gives it."""
    lane = np.arange(64)
    _, jo = P.argmin_first(np.full(64, np.inf, dtype), np.full(64, pc.INT_MAX, I32))
    assert (jo == 0).all(), jo
    _, jo = P.argmin_first(np.full(64, np.nan, dtype), lane + 1)
    assert (jo == 0).all(), jo


@pytest.mark.parametrize("dtype,seed", [pytest.param(F32, 51, id="f32"), pytest.param(F64, 51, id="f64")])
def test_ordered_sum_adds_strictly_in_lane_order(P, dtype, seed):
    v = pc.ordered_sum_input(dtype, seed)
    for first, n in pc.ORDERED_CASES:
        want = pc.sequential_sum(pc.ORDERED_ACC, v, first, n)
        if n >= 8:  # the input discriminates: another association gives other bits (below 8 terms np.sum is this very loop)
            other = dtype(dtype(pc.ORDERED_ACC) + np.sum(v[first:first + n], dtype=dtype))
            assert pc.bits(np.array([other]))[0] != pc.bits(np.array([want]))[0], (first, n)
        got = P.ordered_sum(pc.ORDERED_ACC, v, first, n)
        assert (pc.bits(got) == pc.bits(np.array([want]))[0]).all(), (first, n, got, want)


# ------------------------------------------------------------------------------------------ searches
def _lattice_sweep(P, ref, qx, qy, tag, wlens=pc.WLENS):
    bad = []
    for wlen in wlens:
        for c in pc.starts(wlen):
            d = pc.dist2(ref, c, wlen, qx, qy, F64)  # exact: integers against half-integers
            bad += pc.search_mismatches(P.search(ref, c, wlen, qx, qy), c + np.argmin(d, axis=1), f"{tag} wlen {wlen} c {c}")
    return bad


@pytest.mark.parametrize("dtype", FP)
def test_searches_take_the_first_minimum_on_a_lattice(P, dtype):
    """Integer path coordinates with many duplicates against half-integer queries: every distance is exact whatever the
    contraction, ties abound, and every variant must return c + np.argmin exactly."""
    ref = pc.lattice_path(dtype)
    qx, qy = pc.lattice_queries(dtype)
    bad = _lattice_sweep(P, ref, qx, qy, "lattice")
    assert not bad, bad[:12]


@pytest.mark.parametrize("dtype", FP)
def test_searches_minimum_at_the_first_and_at_the_last_candidate(P, dtype):
    qx, qy = np.full(64, 12.5, dtype), (12.5 + np.arange(64) % 3).astype(dtype)
    bad = []
    for wlen in (1, 3, 7, 33, 65, 199, 255, 256):  # (odd windows: the last candidate sits beside the padding point)
        for c in pc.starts(wlen):
            for at in (0, wlen - 1):
                ref = pc.lattice_path(dtype)
                ref[c + at, :2] = 12.0  # the one candidate near the queries
                res = P.search(ref, c, wlen, qx, qy)
                bad += pc.search_mismatches(res, np.full(64, c + at), f"min at {at} wlen {wlen} c {c}")
    ref = pc.lattice_path(dtype)
    ref[:, 0], ref[:, 1] = 3.0, -2.0  # all candidates identical: the first one
    bad += _lattice_sweep(P, ref, *pc.lattice_queries(dtype), "identical", wlens=(1, 2, 7, 33, 64, 65, 200, 256))
    assert not bad, bad[:12]


@pytest.mark.parametrize("dtype", FP)
def test_searches_pick_a_nearest_candidate_on_real_data(P, dtype):
    """The chosen candidate's f64 distance is within (1 + 2^-20) of the f64 minimum for float (at most five roundings per
    distance across two distances), (1 + 2^-49) for double and for the x0 search, whose distances are f64 in any build."""
    rng = np.random.default_rng(23)
    ref = np.zeros((pc.N_REF, 4), dtype)
    ref[:, :2] = np.cumsum(rng.normal(0, 0.3, (pc.N_REF, 2)), axis=0)
    qx, qy = rng.normal(0, 3, 64).astype(dtype), rng.normal(0, 3, 64).astype(dtype)
    worst = {}
    for wlen in (1, 7, 33, 64, 65, 200, 256):
        for c in pc.starts(wlen):
            d = pc.dist2(ref, c, wlen, qx, qy, F64)
            res = P.search(ref, c, wlen, qx, qy)
            assert res["lanes_agree"].all()
            for row in pc.SEARCH_ROWS[:-1]:
                n = pc.search_valid_lanes(row)
                j = res[row][:n] - c
                assert ((j >= 0) & (j < wlen)).all(), (row, wlen, c, j)
                ratio = d[np.arange(n), j] / d[:n].min(axis=1)
                worst[row] = max(worst.get(row, 1.0), float(ratio.max()))
    print("chosen / minimum f64 distance - 1:", {k: v - 1.0 for k, v in worst.items()})
    for row, w in worst.items():
        assert w <= 1 + (2.0 ** -20 if dtype == F32 and row != "x0" else 2.0 ** -49), (row, w - 1.0)


@pytest.fixture(scope="module")
def nonfinite(P):
    """{dtype: [(tag, result rows, want[64])]}: computed once, shared by the variants' tests below"""
    out = {}
    for dtype in (F32, F64):
        ref = pc.lattice_path(dtype)
        qx, qy = pc.nonfinite_queries(dtype)
        runs = []
        for wlen in (1, 7, 64, 65, 200):
            for c in (0, 5):
                want = {t: c + np.argmin(pc.dist2(ref, c, wlen, qx, qy, t), axis=1) for t in (dtype, F64)}
                assert (want[dtype] == c).all()  # np.argmin over all-NaN / all-inf distances: the first candidate
                runs.append((f"wlen {wlen} c {c}", P.search(ref, c, wlen, qx, qy), want))
        out[dtype] = runs
    return out


@pytest.mark.parametrize("dtype", FP)
@pytest.mark.parametrize("variant", ["window", "lds", "split", "uniform", "x0"])
def test_searches_stay_in_the_window_for_non_finite_positions(nonfinite, variant, dtype):
    """(NaN, 0), (0, NaN), (inf, 0), (0, -inf) and, for float, (1e20, 0), whose squared distance overflows: no candidate
    compares smaller, and every search returns c -- np.argmin over the same distances in the same type (the x0 search
    computes them in f64, where 1e20 is an ordinary far-away position)."""
    bad = []
    for tag, res, want in nonfinite[dtype]:
        for row in pc.SEARCH_ROWS[:-1]:
            if not row.startswith(variant):
                continue
            n = pc.search_valid_lanes(row)
            w = want[F64 if row == "x0" else dtype][:n]
            if not np.array_equal(res[row][:n], w):
                lane = int(np.nonzero(res[row][:n] != w)[0][0])
                bad.append(f"{row} {tag}: lane {lane} got {int(res[row][lane])}, want {int(w[lane])}")
    assert not bad, bad[:8]


# ------------------------------------------------------------------------------------------ collision
@pytest.mark.parametrize("dtype", FP)
@pytest.mark.parametrize("n_obs", pc.N_OBS)
def test_collision_tests_agree_with_f64_outside_the_margin(P, n_obs, dtype):
    """Outline (WIDE and point by point) against the eight outline points in f64, circle against the centre.  Poses whose
    f64 margin |min d^2 - r^2| / r^2 exceeds 1e-4 must agree exactly; flips are allowed only inside it."""
    res = pc.collision_check(P, n_obs, dtype)
    print(n_obs, res)
    for name, r in res.items():
        assert r["frac_outside"] >= 0.95 and 0.0 < r["frac_hit"] < 1.0, (name, r)  # the scene discriminates (f64 alone)
        assert r["flips_outside"] == 0, (name, r)


# ------------------------------------------------------------------------------------------ look-back pieces
def _lb_mismatches(tag, got_m, got_bad, m, bad, where=None):
    where = np.ones(m.size, bool) if where is None else where
    wrong = where & ((got_m != m) | (got_bad != bad))
    return [f"{tag}: call {i} got m {int(got_m[i])} bad {int(got_bad[i])}, want {int(m[i])} {int(bad[i])}"
            for i in np.nonzero(wrong)[0][:4]]


@pytest.mark.parametrize("dtype", FP)
def test_lb_scan_on_a_lattice_bitwise(P, dtype):
    """Exact distances: ties between consecutive candidates (no descent), positions on a candidate, rows that fold back (bad),
    a descent at the first candidate only, at the last only, at all 32, absent candidates from nc on -- m and bad of every
    call, one and two positions per lane."""
    pos = pc.lb_lattice_positions().astype(dtype)
    wrong = []
    for name, row in pc.lb_lattice_rows().items():
        cand = row.astype(dtype)
        m, bad, _, _ = pc.lb_scan_reference(cand, pos)
        m1, bad1 = P.lb_scan(1, cand, pos)
        m2, bad2 = P.lb_scan(2, cand, pos)
        wrong += _lb_mismatches(f"{name} NP=1", m1, bad1, m, bad) + _lb_mismatches(f"{name} NP=2", m2, bad2, m, pc.lb_pairs_bad(bad))
        assert np.array_equal(m1, m2), name
    assert not wrong, wrong[:12]


@pytest.mark.parametrize("dtype", FP)
def test_lb_scan_non_finite_positions(P, dtype):
    """An idle position (x = NaN) counts nothing: m = -1 and no flag.  (inf, 0), (0, NaN) and, for float, (1e20, 0), whose
    squared distance overflows: m stays in [-1, 31] and equals the reference's bits."""
    pos = pc.lb_nonfinite_positions(dtype)
    for name in ("line", "fold", "line_nc5"):
        cand = pc.lb_lattice_rows()[name].astype(dtype)
        m, bad, _, _ = pc.lb_scan_reference(cand, pos)
        assert m[0] == -1 and not bad[0]
        for positions_per_lane in (1, 2):
            gm, gb = P.lb_scan(positions_per_lane, cand, pos)
            assert ((gm >= -1) & (gm <= 31)).all(), (name, gm)
            assert np.array_equal(gm, m), (name, positions_per_lane, gm, m)
            assert np.array_equal(gb, bad if positions_per_lane == 1 else pc.lb_pairs_bad(bad)), (name, positions_per_lane, gb)


@pytest.mark.parametrize("dtype", FP)
def test_lb_scan_on_real_data_outside_the_margin(P, dtype):
    """Positions scattered (sigma 0.3) around a gently curved stretch of 32 candidates: every call whose consecutive candidate
    distances differ by more than LB_GAP relative in f64 must give the reference's m and bad; at most 2 % may be left out."""
    cand, pos, m, bad, compared = pc.lb_real_reference(dtype)
    left_out = 1.0 - float(compared.mean())
    print("lb_scan real data: share left out", left_out)
    assert left_out <= pc.LB_LEFT_OUT_MAX
    m1, bad1 = P.lb_scan(1, cand, pos)
    m2, bad2 = P.lb_scan(2, cand, pos)
    assert np.array_equal(m1, m2)
    wrong = _lb_mismatches("NP=1", m1, bad1, m, bad, compared)
    pair_ok = pc.lb_pairs_bad(~compared) == 0  # a pair's flag is compared where both of its calls are
    wrong += _lb_mismatches("NP=2", m2, bad2, m, pc.lb_pairs_bad(bad), compared & pair_ok)
    assert not wrong, wrong


def test_lb_reach_is_the_exactness_argument(P):
    table, want = pc.lb_reach_table()
    assert 0.2 < want.mean() < 0.8  # (the table discriminates)
    got = P.lb_reach(table)
    assert np.array_equal(got, want), table[got != want][:8]


def test_lb_tag_keeps_the_low_byte_free_and_aliases_after_2_24(P):
    seq = np.array([1, 0xFFFFFF, 0x1000001, 0xFFFFFFFF], np.uint64)
    tag = P.lb_tag(seq)
    assert np.array_equal(tag, pc.lb_tag_reference(seq).astype(U32))
    assert ((tag & 0xFF) == 0).all() and (tag != 0).all()
    assert tag[2] == tag[0]  # the aliasing period: 2^24 launch pairs


LB_TAG = 0x00ABCD00


@pytest.mark.parametrize("B", pc.LB_EXCHANGE_B)
def test_lb_exchange_of_fresh_words(P, B):
    """Every workgroup publishes: b reads the largest offset and any bad bit of [0, b), workgroup 0 nothing, and all 8 copies
    hold the words.  (256 / 257: the lane's second 16-byte load; 4 / 5: the four words of a lane.)"""
    for name, marks in pc.lb_exchange_marks(B).items():
        words, off, badbit = pc.lb_exchange_words(B, LB_TAG, marks)
        published = np.ones(B, bool)
        want_ok, want_E, want_bad = pc.lb_exchange_reference(off, badbit, published)
        assert want_ok.all() and want_E[0] == 0 and not want_bad[0]
        ok, E, bad, slots = P.lb_exchange(words, ~published, LB_TAG, P.lb_default_limit(), pc.lb_slots(0))
        assert ok.all(), (name, np.nonzero(~ok)[0][:8])
        assert np.array_equal(E, want_E), (name, np.nonzero(E != want_E)[0][:8])
        assert np.array_equal(bad, want_bad), (name, np.nonzero(bad != want_bad)[0][:8])
        assert pc.lb_published_everywhere(slots, words, published), name


@pytest.mark.parametrize("B", [5, 16])
def test_lb_exchange_never_takes_a_stale_word(P, B):
    """The buffer holds words of another launch pair -- offset 127, bad bit -- and workgroup s never publishes: everyone up to
    s reads fresh words only, everyone behind s gives up after 2000 ticks (20 us)."""
    stale = pc.lb_slots((LB_TAG ^ 0x5500) | pc.LB_BAD | 127)
    for s in (0, 3, B - 1):
        words, off, badbit = pc.lb_exchange_words(B, LB_TAG, [])
        off = np.minimum(off, 100)  # (below the stale offset, so that a leak shows)
        words = ((words & pc.LB_TAG_MASK) | off).astype(U32)
        published = np.arange(B) != s
        want_ok, want_E, want_bad = pc.lb_exchange_reference(off, badbit, published)
        assert np.array_equal(want_ok, np.arange(B) <= s) and not want_bad.any()
        ok, E, bad, slots = P.lb_exchange(words, ~published, LB_TAG, 2000, stale)
        assert np.array_equal(ok, want_ok), (s, ok)
        assert np.array_equal(E, want_E) and np.array_equal(bad, want_bad), (s, E, bad)
        assert pc.lb_published_everywhere(slots, words, published), s
        assert (slots.reshape(pc.LB_COPIES, -1)[:, s] == stale[0]).all(), s


def test_lb_exchange_with_limit_0_gives_up_before_the_first_poll(P):
    for B in (1, 9):
        words, off, badbit = pc.lb_exchange_words(B, LB_TAG, [])
        ok, E, bad, slots = P.lb_exchange(words, np.zeros(B, I32), LB_TAG, 0, pc.lb_slots(0))
        assert np.array_equal(ok, np.arange(B) == 0), ok
        assert (E == 0).all() and not bad.any()
        assert pc.lb_published_everywhere(slots, words, np.ones(B, bool))


# ------------------------------------------------------------------------------------------ sampler
def test_philox_known_answers_and_random_counters_bitwise(P):
    ctr, key, want = (np.array([k[i] for k in pc.KAT], U32) for i in range(3))
    assert np.array_equal(P.philox(ctr, key), want)
    rng = np.random.default_rng(61)
    ctr = rng.integers(0, 2 ** 32, (4096, 4), dtype=np.uint64).astype(U32)
    key = rng.integers(0, 2 ** 32, (4096, 2), dtype=np.uint64).astype(U32)
    assert np.array_equal(P.philox(ctr, key), pc.oracle_philox(ctr, key))


def test_uniform_open_bitwise(P):
    r = np.array(pc.WORDS, U32)
    want = philox.uniform_open(r)
    assert np.array_equal(want.astype(F32).astype(F64), want)  # exact in f32
    assert np.array_equal(pc.bits(P.uniform_open(r)), pc.bits(want.astype(F32)))


def test_box_muller_at_the_edge_words(P):
    err = pc.box_muller_abs_err(P)
    print("box_muller max abs error", err.max())
    assert err.max() <= 4e-6, err.max()  # the atol of test_sampler_matches_numpy_restatement for this sigma


def test_sample_at_the_counter_edges(P):
    seed, it, stream = 0x1234567890ABCDEF, 2 ** 32 - 1, 7
    ts = np.array([0, 1, 2, 3, 98, 99])
    for k in (0, 2 ** 32 - 1):
        got = P.sample(seed, it, np.full(ts.size, k, np.uint64).astype(U32), ts, stream, pc.chol_f32())
        want = philox.sample_epsilon(pc.SIGMA, seed, it, 1, 100, k_offset=k, stream=stream)[0, ts]
        np.testing.assert_allclose(got, want, rtol=0, atol=4e-6)


@pytest.mark.parametrize("T", (1, 2, 7, 64))
def test_noise_pair_equals_noise_at_bitwise(P, T):
    """A lane's two steps from one Philox block, or two loads: the values noise_at gives at steps 2l and 2l+1, bit for bit, on
    both branches; an odd horizon leaves the last lane's second step beyond it, where the pair comes back 0."""
    seed, it = 0x1234567890ABCDEF, 5
    row = np.random.default_rng(71).standard_normal((T, 2)).astype(F32)
    steps = np.zeros((64, 2, 2), F32)  # the row as the lanes own it: [l][step][channel], 0 beyond the horizon
    steps.reshape(128, 2)[:T] = row
    for k in (0, 1, 2 ** 20 + 3):
        for k_offset in (0, 5):
            for agent in (0, 3):
                for philox_branch in (True, False):
                    pair, single = P.noise_pair(philox_branch, seed, it, T, k_offset, 0, agent, k, pc.chol_f32(), row)
                    tag = (k, k_offset, agent, philox_branch)
                    assert np.array_equal(pc.bits(pair), pc.bits(single)), tag
                    assert not pair.reshape(128, 2)[T:].any(), tag
                    assert pair.reshape(128, 2)[:T].all(), tag  # (a draw is never exactly 0, nor is the row)
                    if not philox_branch:
                        assert np.array_equal(pc.bits(pair), pc.bits(steps)), tag
