"""Inputs, f64 references and comparisons for the device primitives (mathfn.h, wave_ops.h, philox.h, mppi_device.h -- the
pieces of the one-launch waypoint index, lb_*, among them) as
tests/device/prims_harness.hip exposes them.  TEST INFRASTRUCTURE: tests/test_gpu_primitives.py asserts on what these
functions return, tools/prims_report.py prints the same figures.

Every reference is NumPy in f64, computed from the f32 input widened to f64.  "ulp" is the spacing of the f64 result
rounded to f32.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from oracle import philox

F32, F64, I32, U32 = np.float32, np.float64, np.int32, np.uint32
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
SCAN, HALF, ROW, SEG1, SEG2, REDUCE = range(6)
SEG_LEN = {SCAN: 64, HALF: 32, ROW: 16, SEG1: 64, SEG2: 32}
SEARCH_ROWS = ("window", "lds", "split2", "split4", "split8", "split16", "uniform", "x0", "lanes_agree")
WORDS = (0, 0x1FF, 0x200, 0x7FFFFFFF, 0x80000000, 0xFFFFFE00, 0xFFFFFFFF)
SIGMA = np.array([[0.5, 0.1], [0.1, 0.2]])


# the words of the one-launch waypoint index (mppi_kernels.h)
LB_CAND, LB_BAD, LB_COPIES, LB_COPY_STRIDE = 32, 0x80, 8, 2048
LB_SLOT_WORDS, LB_TAG_MASK, LB_MAX_BLOCKS = LB_COPIES * LB_COPY_STRIDE, 0xFFFFFF00, 512
LB_ABSENT = 1e30  # a candidate beyond the path's end, as the kernels stage it

def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _sfx(dtype):
    return {F32: "f32", F64: "f64", I32: "i32"}[np.dtype(dtype).type]


class Prims:
    """ctypes front of libmppi_prims.so: NumPy in, NumPy out; a HIP error raises."""

    def __init__(self, path):
        self.lib = C.CDLL(path)
        assert self.lib.prims_search_rows() == len(SEARCH_ROWS)

    def _call(self, name, *args):
        fn = getattr(self.lib, name)
        fn.restype = C.c_int
        err = fn(*args)
        if err != 0:
            raise RuntimeError(f"{name}: hipError_t {err}")

    # ---- mathfn
    def _map(self, name, x, dtype, *extra, outs=1):
        x = np.ascontiguousarray(x, dtype)
        o = [np.empty_like(x) for _ in range(outs)]
        self._call(name, _p(x), *extra, *[_p(a) for a in o], C.c_int(x.size))
        return o[0] if outs == 1 else tuple(o)

    def sincos(self, x):
        return self._map("prims_sincos_f32", x, F32, outs=2)

    def tan(self, x):
        return self._map("prims_tan_f32", x, F32)

    def pymod(self, a, m):
        return self._map("prims_pymod_f32", a, F32, C.c_float(m))

    def exp(self, x):
        return self._map("prims_exp_f32", x, F32)

    def clamp(self, v, lim, dtype):
        ct = C.c_float if dtype == F32 else C.c_double
        return self._map("prims_clamp_" + _sfx(dtype), v, dtype, ct(lim))

    # ---- wave_ops (one wave: 64 values)
    def _wave(self, name, x, *pre, out_n=64):
        x = np.ascontiguousarray(x)
        assert x.shape == (64,)
        o = np.empty(out_n, x.dtype)
        self._call(name + _sfx(x.dtype), *pre, _p(x), _p(o))
        return o

    def scan(self, op, variant, x):
        return self._wave("prims_scan_", x, C.c_int(op), C.c_int(variant))

    def shift(self, variant, x, carry):
        x = np.ascontiguousarray(x)
        ct = C.c_float if x.dtype == F32 else C.c_double
        o = np.empty(64, x.dtype)
        self._call("prims_shift_" + _sfx(x.dtype), C.c_int(variant), _p(x), ct(carry), _p(o))
        return o

    def read_lane(self, x):
        return self._wave("prims_read_lane_", x, out_n=64 * 64).reshape(64, 64)

    def shfl_xor(self, m, x):
        return self._wave("prims_shfl_xor_", x, C.c_int(m))

    def argmin_first(self, d, j):
        d, j = np.ascontiguousarray(d), np.ascontiguousarray(j, I32)
        do, jo = np.empty_like(d), np.empty_like(j)
        self._call("prims_argmin_" + _sfx(d.dtype), _p(d), _p(j), _p(do), _p(jo))
        return do, jo

    def ordered_sum(self, acc, v, first, n):
        v = np.ascontiguousarray(v)
        ct = C.c_float if v.dtype == F32 else C.c_double
        o = np.empty(64, v.dtype)
        self._call("prims_ordered_sum_" + _sfx(v.dtype), ct(acc), _p(v), C.c_int(first), C.c_int(n), _p(o))
        return o

    # ---- searches: {row name: int32[64]}
    def search(self, ref, c, wlen, qx, qy):
        ref = np.ascontiguousarray(ref)
        qx, qy = np.ascontiguousarray(qx, ref.dtype), np.ascontiguousarray(qy, ref.dtype)
        assert ref.ndim == 2 and ref.shape[1] == 4 and qx.shape == qy.shape == (64,)
        o = np.empty((len(SEARCH_ROWS), 64), I32)
        self._call("prims_search_" + _sfx(ref.dtype), _p(ref), C.c_int(ref.shape[0]), C.c_int(c), C.c_int(wlen), _p(qx),
                   _p(qy), _p(o))
        return dict(zip(SEARCH_ROWS, o))

    # ---- collision: bool[3][n] = outline WIDE, outline point by point, circle
    def collide(self, obs, shape, poses):
        obs = np.ascontiguousarray(obs)
        shape, poses = np.ascontiguousarray(shape, obs.dtype), np.ascontiguousarray(poses, obs.dtype)
        assert obs.shape[1] == 4 and shape.shape == (2, 9) and poses.shape[1] == 3
        o = np.empty((3, poses.shape[0]), I32)
        self._call("prims_collide_" + _sfx(obs.dtype), C.c_int(obs.shape[0]), _p(obs), _p(shape), _p(poses),
                   C.c_int(poses.shape[0]), _p(o))
        assert set(np.unique(o)) <= {0, 1}
        return o.astype(bool)

    # ---- look-back pieces (lb_* of mppi_device.h)
    def lb_scan(self, positions_per_lane, cand, pos):
        """candidates [32][2], positions [n][2] -> (m int32[n], bad bool[n]); two positions per lane: n is padded with an idle
        position (x = NaN) to an even count, and `bad` is the lane's flag at both of its positions"""
        cand = np.ascontiguousarray(cand)
        pos = np.ascontiguousarray(pos, cand.dtype)
        assert cand.shape == (LB_CAND, 2) and pos.ndim == 2 and pos.shape[1] == 2
        n = pos.shape[0]
        if n % positions_per_lane:
            pos = np.concatenate([pos, np.array([[np.nan, 0.0]], cand.dtype)])
        m, bad = np.empty(pos.shape[0], I32), np.empty(pos.shape[0], I32)
        self._call("prims_lb_scan_" + _sfx(cand.dtype), C.c_int(positions_per_lane), _p(cand), _p(pos), C.c_int(pos.shape[0]),
                   _p(m), _p(bad))
        assert set(np.unique(bad)) <= {0, 1}
        return m[:n], bad[:n].astype(bool)

    def lb_reach(self, table):
        table = np.ascontiguousarray(table, I32)
        assert table.ndim == 2 and table.shape[1] == 4
        o = np.empty(table.shape[0], I32)
        self._call("prims_lb_reach", _p(table), C.c_int(table.shape[0]), _p(o))
        assert set(np.unique(o)) <= {0, 1}
        return o.astype(bool)

    def lb_tag(self, seq):
        seq = np.ascontiguousarray(seq, U32)
        o = np.empty(seq.size, U32)
        self._call("prims_lb_tag", _p(seq), C.c_int(seq.size), _p(o))
        return o

    def lb_default_limit(self):
        return int(self.lib.prims_lb_default_limit())

    def lb_exchange(self, words, skip, tag, limit, slots):
        """B one-wave workgroups in one launch -> (ok bool[B], E int[B], bad bool[B], slots after the launch)"""
        words, skip = np.ascontiguousarray(words, U32), np.ascontiguousarray(skip, I32)
        slots = np.array(slots, U32)  # (a copy: the call returns the buffer in place)
        assert self.lib.prims_lb_slot_words() == LB_SLOT_WORDS == slots.size and words.shape == skip.shape
        o = np.empty((words.size, 4), I32)
        self._call("prims_lb_exchange", C.c_int(words.size), _p(words), _p(skip), C.c_uint(int(tag)), C.c_int(limit), _p(slots),
                   _p(o))
        assert (o[:, 3] == 1).all(), "the lanes of a wave disagree on what lb_wait returned"
        assert set(np.unique(o[:, [0, 2]])) <= {0, 1}
        return o[:, 0].astype(bool), o[:, 1].copy(), o[:, 2].astype(bool), slots

    # ---- sampler
    def philox(self, ctr, key):
        ctr, key = np.ascontiguousarray(ctr, U32), np.ascontiguousarray(key, U32)
        assert ctr.shape[1] == 4 and key.shape == (ctr.shape[0], 2)
        o = np.empty_like(ctr)
        self._call("prims_philox", _p(ctr), _p(key), _p(o), C.c_int(ctr.shape[0]))
        return o

    def uniform_open(self, r):
        r = np.ascontiguousarray(r, U32)
        o = np.empty(r.size, F32)
        self._call("prims_uniform_open", _p(r), _p(o), C.c_int(r.size))
        return o

    def box_muller(self, ra, rb, chol):
        ra, rb, chol = np.ascontiguousarray(ra, U32), np.ascontiguousarray(rb, U32), np.ascontiguousarray(chol, F32)
        o = np.empty((ra.size, 2), F32)
        self._call("prims_box_muller", _p(ra), _p(rb), _p(chol), _p(o), C.c_int(ra.size))
        return o

    def sample(self, seed, iteration, k, t, stream, chol):
        k, t, chol = np.ascontiguousarray(k, U32), np.ascontiguousarray(t, I32), np.ascontiguousarray(chol, F32)
        o = np.empty((k.size, 2), F32)
        self._call("prims_sample", C.c_uint(seed & 0xFFFFFFFF), C.c_uint(seed >> 32), C.c_uint(iteration), _p(k), _p(t),
                   C.c_uint(stream), _p(chol), _p(o), C.c_int(k.size))
        return o

    def noise_pair(self, philox_branch, seed, iteration, T, k_offset, noise_stream, agent, k, chol, row):
        """one wave, lane l = steps 2l, 2l+1 of sample k -> (noise_pair [64][2][2], noise_at [64][2][2]); `row` [T][2] is
        sample k's row of the agent's noise tensor (what the tensor branch reads)"""
        chol, row = np.ascontiguousarray(chol, F32), np.ascontiguousarray(row, F32)
        assert row.shape == (T, 2)
        o = np.empty((64, 8), F32)
        self._call("prims_noise_pair", C.c_int(int(philox_branch)), C.c_uint(seed & 0xFFFFFFFF), C.c_uint(seed >> 32),
                   C.c_uint(iteration), C.c_int(T), C.c_int(k_offset), C.c_int(noise_stream), C.c_int(agent), C.c_int(k),
                   _p(chol), _p(row), _p(o))
        return o[:, :4].reshape(64, 2, 2), o[:, 4:].reshape(64, 2, 2)


# ------------------------------------------------------------------------------------------ mathfn
    # ---- mppi_merge.h
    def merge_record_len(self, dtype, T):
        return int(getattr(self.lib, f"prims_merge_record_len_{_sfx(dtype)}")(C.c_int(T)))

    def merge_combine(self, dtype, nwin, rho, eta, eta2, hits, W, n, beta, want_hits=True, pad=0.0):
        """merge_combine<dtype, 256, nwin> over the first n of the given slots (the slots past n: the caller's absent ones; the
        harness zero-fills up to nwin * 256 + 256).  W [slots, 2T]; ``pad``: what the record words outside {heads, W} hold.
        Returns (rho, eta, eta2, n_hit, w_eps[2T]) in ``dtype``."""
        W = np.asarray(W, np.float64)
        slots, T = W.shape[0], W.shape[1] // 2
        rl = self.merge_record_len(dtype, T)
        heads = np.stack([rho, eta, eta2, hits], axis=1).astype(dtype)
        recs = np.full((slots, rl), pad, dtype)
        recs[:, :3] = heads[:, :3]
        recs[:, 4:4 + 2 * T] = W.astype(dtype)
        heads, recs = np.ascontiguousarray(heads), np.ascontiguousarray(recs)
        out = np.empty(4 + 2 * T, dtype)
        real = C.c_float if np.dtype(dtype) == np.dtype(F32) else C.c_double
        self._call(f"prims_merge_combine_{_sfx(dtype)}", C.c_int(nwin), _p(heads), _p(recs), C.c_int(slots), C.c_int(n), C.c_int(T),
                   real(float(dtype(beta))), C.c_int(int(bool(want_hits))), _p(out))
        return out[0], out[1], out[2], out[3], out[4:]

    def merge_abi(self, dtype, rho, eta, eta2, W, beta):
        """merge_abi<dtype> over n records {rho, eta, eta2, W[2T]} in doubles.  Returns (rho, eta, eta2, w_eps[2T])."""
        W = np.asarray(W, np.float64)
        n, T = W.shape[0], W.shape[1] // 2
        recs = np.ascontiguousarray(np.concatenate([np.stack([rho, eta, eta2], axis=1), W], axis=1), dtype=np.float64)
        out = np.empty(3 + 2 * T, dtype)
        real = C.c_float if np.dtype(dtype) == np.dtype(F32) else C.c_double
        self._call(f"prims_merge_abi_{_sfx(dtype)}", _p(recs), C.c_int(n), C.c_int(T), real(float(dtype(beta))), _p(out))
        return out[0], out[1], out[2], out[3:]


def ulp_err(got, want64):
    """|got - want| in units of the spacing of want rounded to f32."""
    w32 = want64.astype(F32)
    return np.abs(got.astype(F64) - want64) / np.spacing(np.abs(w32)).astype(F64)


def neighbours(x32):
    x32 = np.asarray(x32, F32)
    return np.concatenate([np.nextafter(x32, F32(-np.inf)), x32, np.nextafter(x32, F32(np.inf))])


def sincos_inputs():
    """(polynomial-branch inputs, library-branch inputs)"""
    rng = np.random.default_rng(11)
    k = np.arange(-20860, 20861, dtype=F64)
    poly = np.concatenate([rng.uniform(-32768.0, 32768.0, 1 << 20).astype(F32), neighbours((k * (np.pi / 2)).astype(F32)),
                           np.array([0.0, -0.0, 1e-40, 32768.0, -32768.0], F32)])
    assert np.abs(poly).max() <= 32768.0
    lib = np.array([np.nextafter(F32(32768.0), F32(np.inf)), 1e5, 1e6, 3e7, 1e9], F32)
    return poly, lib


def sincos_errors(P):
    """max ulp error of the polynomial branch (sin, cos) and max absolute error of the library branch"""
    poly, lib = sincos_inputs()
    s, c = P.sincos(poly)
    x = poly.astype(F64)
    es, ec = ulp_err(s, np.sin(x)), ulp_err(c, np.cos(x))
    ls, lc = P.sincos(lib)
    xl = lib.astype(F64)
    return {"sin_ulp": float(es.max()), "sin_worst_x": float(poly[es.argmax()]), "cos_ulp": float(ec.max()),
            "cos_worst_x": float(poly[ec.argmax()]),
            "library_abs": float(max(np.abs(ls - np.sin(xl)).max(), np.abs(lc - np.cos(xl)).max()))}


TAN_BRANCH = F32(0.78539816)


def tan_inputs():
    """(inputs of the polynomial branch, the two arguments just outside it)"""
    rng = np.random.default_rng(12)
    q = F32(np.pi / 4)
    inside = np.concatenate([rng.uniform(-q, q, 1 << 20).astype(F32), np.array([0.523, -0.523, 0.0, -0.0, 1e-40], F32),
                             [TAN_BRANCH, np.nextafter(TAN_BRANCH, F32(0)), -TAN_BRANCH, -np.nextafter(TAN_BRANCH, F32(0))]]).astype(F32)
    inside = inside[np.abs(inside) <= TAN_BRANCH]
    up = np.nextafter(TAN_BRANCH, F32(np.inf))
    return inside, np.array([up, -up], F32)


def tan_errors(P):
    inside, outside = tan_inputs()
    ei = ulp_err(P.tan(inside), np.tan(inside.astype(F64)))
    eo = ulp_err(P.tan(outside), np.tan(outside.astype(F64)))
    return {"tan_ulp": float(ei.max()), "tan_worst_x": float(inside[ei.argmax()]), "tan_outside_ulp": float(eo.max())}


PYMOD_M = F32(2 * np.pi)


def pymod_inputs():
    rng = np.random.default_rng(13)
    k = np.arange(-6000, 6001, dtype=F64)
    m = PYMOD_M
    return np.concatenate([rng.uniform(-40000.0, 40000.0, 1 << 20).astype(F32), neighbours((k * F64(m)).astype(F32)),
                           np.array([0.0, -0.0, -1e-8, -1e-30, m, -m, np.nextafter(m, F32(0))], F32)])


def pymod_check(P):
    """(results, inputs, circular distance to np.mod in f64)"""
    a = pymod_inputs()
    r = P.pymod(a, float(PYMOD_M))
    want = np.mod(a.astype(F64), F64(PYMOD_M))
    d = np.abs(r.astype(F64) - want)
    return r, a, np.minimum(d, F64(PYMOD_M) - d)


def exp_inputs():
    rng = np.random.default_rng(14)
    return np.concatenate([rng.uniform(-87.0, 0.0, (1 << 16) - 2), [-87.0, 0.0]]).astype(F32)


def exp_rel_err(P):
    """(relative error, its bound (2|x| + 4) 2^-24) over [-87, 0]"""
    x = exp_inputs()
    want = np.exp(x.astype(F64))
    return np.abs(P.exp(x).astype(F64) - want) / want, (2 * np.abs(x.astype(F64)) + 4) * 2.0 ** -24


# ------------------------------------------------------------------------------------------ wave_ops
def scan_reference(op, variant, x):
    """op: 'add' | 'min' | 'max' (in x's own type: the inputs are integer-valued, so every association gives the same bits)"""
    acc = {"add": np.cumsum, "min": np.minimum.accumulate, "max": np.maximum.accumulate}[op]
    if variant == REDUCE:
        return np.full(64, acc(x)[-1], x.dtype)
    seg = SEG_LEN[variant]
    return np.concatenate([acc(x[i:i + seg]) for i in range(0, 64, seg)]).astype(x.dtype)


def scan_input(dtype, op, seed):
    rng = np.random.default_rng(seed)
    if dtype == I32:
        x = rng.integers(INT_MIN, INT_MAX, 64, dtype=np.int64, endpoint=True).astype(I32)
        x[rng.choice(64, 6, replace=False)] = [INT_MIN, INT_MAX, INT_MIN, INT_MAX, 0, -1]
        return x
    if dtype == F64:  # below 2^45: both 32-bit halves of the DPP move carry information, and 64 of them add exactly
        x = rng.integers(-(1 << 45) + 1, 1 << 45, 64).astype(F64)
    else:
        x = rng.integers(-(1 << 17) + 1, 1 << 17, 64).astype(F32)
    if op == "min":
        x[rng.choice(64, 4, replace=False)] = [np.inf, -np.inf, np.inf, np.inf]
    return x


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def sequential_sum(acc, v, first, n):
    acc = v.dtype.type(acc)
    for i in range(first, first + n):
        acc = v.dtype.type(acc + v[i])
    return acc


def ordered_sum_input(dtype, seed):
    rng = np.random.default_rng(seed)
    return (rng.choice([-1.0, 1.0], 64) * 2.0 ** rng.uniform(-20, 20, 64)).astype(dtype)


ORDERED_CASES = ((0, 0), (0, 1), (0, 7), (0, 8), (0, 9), (3, 17), (0, 63), (0, 64), (5, 59))
ORDERED_ACC = 0.375


# ------------------------------------------------------------------------------------------ searches
N_REF = 300
WLENS = (1, 2, 3, 7, 8, 31, 32, 33, 63, 64, 65, 199, 200, 255, 256)


def starts(wlen):
    return sorted({0, 5, N_REF - wlen})


def lattice_path(dtype, seed=21):
    rng = np.random.default_rng(seed)
    ref = np.zeros((N_REF, 4), dtype)
    ref[:, :2] = rng.integers(-8, 9, (N_REF, 2))
    ref[:, 2:] = rng.normal(size=(N_REF, 2))  # yaw, v: never read by a search
    return ref


def lattice_queries(dtype, seed=22):
    rng = np.random.default_rng(seed)
    q = rng.integers(-10, 10, (2, 64)) + 0.5
    return q[0].astype(dtype), q[1].astype(dtype)


def dist2(ref, c, wlen, qx, qy, dtype):
    """d[query][candidate] of the window in `dtype` (product and sum rounded separately)"""
    with np.errstate(over="ignore", invalid="ignore"):
        dx = qx.astype(dtype)[:, None] - ref[c:c + wlen, 0].astype(dtype)[None, :]
        dy = qy.astype(dtype)[:, None] - ref[c:c + wlen, 1].astype(dtype)[None, :]
        return dx * dx + dy * dy


def search_valid_lanes(row):
    return 64 // int(row[5:]) if row.startswith("split") else 64


def search_mismatches(res, want, tag):
    """rows of one launch whose stored indices differ from want[64] (the lanes that hold a result)"""
    bad = []
    for row in SEARCH_ROWS[:-1]:
        n = search_valid_lanes(row)
        if not np.array_equal(res[row][:n], want[:n]):
            lane = int(np.nonzero(res[row][:n] != want[:n])[0][0])
            bad.append(f"{row} {tag}: lane {lane} got {int(res[row][lane])}, want {int(want[lane])}")
    if not res["lanes_agree"].all():
        bad.append(f"lanes_agree {tag}: the lanes of a wave-level search disagree")
    return bad


NONFINITE = ((np.nan, 0.0), (0.0, np.nan), (np.inf, 0.0), (0.0, -np.inf), (1e20, 0.0))


def nonfinite_queries(dtype):
    q = NONFINITE if dtype == F32 else NONFINITE[:4]  # 1e20: d^2 overflows in f32 only
    q = np.array([q[i % len(q)] for i in range(64)], dtype)
    return q[:, 0].copy(), q[:, 1].copy()


# ------------------------------------------------------------------------------------------ collision
N_POSES = 4096
# the reference's outline (mppi_race_car_obstacle.py:256-264): vehicle 4.0 x 3.0, safety margin rate 1.5
_VL, _VW = 4.0 * 1.5, 3.0 * 1.5
SHAPE = np.array([[-0.5 * _VL, -0.5 * _VL, 0.0, 0.5 * _VL, 0.5 * _VL, 0.5 * _VL, 0.0, -0.5 * _VL, -0.5 * _VL],
                  [0.0, 0.5 * _VW, 0.5 * _VW, 0.5 * _VW, 0.0, -0.5 * _VW, -0.5 * _VW, -0.5 * _VW, 0.0]])
COLLISION_MARGIN = 1e-4
COLLISION_SEED = 31
N_OBS = (1, 2, 64, 65, 70)


def collision_scene(n_obs, dtype, seed=COLLISION_SEED):
    """obs[n_obs][4] = {x, y, r^2, 0}, poses[4096][3]; the first poses sit on the fold boundaries of the WIDE form: yaw = 0,
    +-pi/2, pi and circle centres on the body axes"""
    rng = np.random.default_rng(seed + n_obs)
    r = np.clip(4.0 / np.sqrt(n_obs), 0.4, 2.5) * rng.uniform(0.7, 1.3, n_obs)
    obs = np.zeros((n_obs, 4))
    obs[:, :2] = rng.uniform(-10, 10, (n_obs, 2))
    obs[:, 2] = r * r
    poses = np.column_stack([rng.uniform(-14, 14, N_POSES), rng.uniform(-14, 14, N_POSES), rng.uniform(-np.pi, np.pi, N_POSES)])
    i = 0
    for yaw in (0.0, np.pi / 2, -np.pi / 2, np.pi):
        for _ in range(32):
            poses[i, 2] = yaw
            i += 1
    for axis in (0.0, np.pi / 2, np.pi, -np.pi / 2):  # circle 0's centre on the body's +x, +y, -x, -y axis
        for _ in range(32):
            yaw, dist = rng.uniform(-np.pi, np.pi), rng.uniform(0.0, 6.0)
            poses[i] = [obs[0, 0] - dist * np.cos(yaw + axis), obs[0, 1] - dist * np.sin(yaw + axis), yaw]
            i += 1
    return obs.astype(dtype), poses.astype(dtype)


def collision_reference(obs, poses):
    """f64, from the inputs as the device holds them: (hit, margin) for the outline test and for the circle test;
    margin = min over (point, circle) of |d^2 - r^2| / r^2"""
    obs, poses = obs.astype(F64), poses.astype(F64)
    x, y, yaw = poses[:, 0, None], poses[:, 1, None], poses[:, 2, None]
    sx, sy = SHAPE[0, None, :8], SHAPE[1, None, :8]
    px, py = sx * np.cos(yaw) - sy * np.sin(yaw) + x, sx * np.sin(yaw) + sy * np.cos(yaw) + y  # [n][8]
    out = []
    for qx, qy in ((px, py), (x, y)):
        d2 = (qx[:, :, None] - obs[None, None, :, 0]) ** 2 + (qy[:, :, None] - obs[None, None, :, 1]) ** 2
        r2 = obs[None, None, :, 2]
        out.append(((d2 < r2).any(axis=(1, 2)), (np.abs(d2 - r2) / r2).min(axis=(1, 2))))
    return out


def collision_check(P, n_obs, dtype):
    """per variant: flips outside the margin (must be 0), flips inside it, and the reference's own statistics"""
    obs, poses = collision_scene(n_obs, dtype)
    shape = SHAPE.astype(dtype)
    (hit_o, mar_o), (hit_c, mar_c) = collision_reference(obs, poses)
    got = P.collide(obs, shape, poses)
    res = {}
    for name, g, hit, mar in (("outline_wide", got[0], hit_o, mar_o), ("outline_points", got[1], hit_o, mar_o),
                              ("circle", got[2], hit_c, mar_c)):
        flip = g != hit
        res[name] = {"flips_outside": int((flip & (mar > COLLISION_MARGIN)).sum()),
                     "flips_inside": int((flip & (mar <= COLLISION_MARGIN)).sum()),
                     "frac_outside": float((mar > COLLISION_MARGIN).mean()), "frac_hit": float(hit.mean())}
    return res


# ------------------------------------------------------------------------------------------ look-back pieces
F32_OVERFLOW = 2.0 ** 128 - 2.0 ** 103  # from here on a float result rounds to +inf


def lb_distances(cand, pos):
    """d[call][candidate] in f64 from the inputs widened to f64.  For float inputs a distance beyond the format's range is +inf,
    as the device has it (an absent candidate, a position of 1e20); the inputs keep every other distance far below that."""
    c, q = np.asarray(cand).astype(F64), np.asarray(pos).astype(F64)
    with np.errstate(over="ignore", invalid="ignore"):
        d = (q[:, None, 0] - c[None, :, 0]) ** 2 + (q[:, None, 1] - c[None, :, 1]) ** 2
    if np.asarray(cand).dtype == F32:
        fin = d[np.isfinite(d)]
        assert not ((fin > 1e30) & (fin < 1e39)).any()  # (nothing near the threshold, where the order of rounding would matter)
        d = np.where(d >= F32_OVERFLOW, np.inf, d)
    return d


def lb_scan_reference(cand, pos):
    """(m, bad, descent bits[call][32], smallest relative gap between consecutive finite candidate distances per call).
    g_j = d_j < d_(j-1) with d_(-1) = +inf; m = popcount(g) - 1; bad unless the set bits are a prefix.  Where a call has a
    descent and is not bad, m is its first minimum -- asserted here, it is what the kernels rely on."""
    d = lb_distances(cand, pos)
    with np.errstate(invalid="ignore"):
        prev = np.concatenate([np.full((d.shape[0], 1), np.inf), d[:, :-1]], axis=1)
        g = d < prev
        both = np.isfinite(d) & np.isfinite(prev)
        gap = np.where(both, np.abs(d - prev) / np.maximum(np.maximum(d, prev), np.finfo(F64).tiny), np.inf).min(axis=1)
    pcnt = g.sum(axis=1)
    m = (pcnt - 1).astype(I32)
    bad = (g[:, 1:] & ~g[:, :-1]).any(axis=1)  # a descent behind a non-descent
    good = ~bad & (pcnt > 0)
    assert (m[good] == np.argmin(d[good], axis=1)).all()
    return m, bad, g, gap


def lb_pairs_bad(bad):
    """the flag of a lane that owns positions 2i and 2i + 1, at both of them"""
    b = np.concatenate([bad, [False] * (bad.size % 2)]).reshape(-1, 2).any(axis=1)
    return np.repeat(b, 2)[:bad.size]


def _row(xy, nc=LB_CAND):
    r = np.full((LB_CAND, 2), LB_ABSENT)
    r[:nc] = np.asarray(xy, F64)[:nc]
    return r


def lb_lattice_rows():
    """{name: candidates[32][2]}: integers and quarters, so that every distance and every comparison is exact in float"""
    j = np.arange(LB_CAND, dtype=F64)
    line = np.stack([j, np.zeros(LB_CAND)], 1)
    rows = {"line": line}
    # every second candidate repeats the one before it: exact ties between consecutive candidates
    rows["ties"] = np.stack([np.floor(j / 2), np.zeros(LB_CAND)], 1)
    # out for 16 candidates, back beside them for 16: the descents resume after a rise
    rows["fold"] = np.stack([np.where(j < 16, j, 31 - j), np.where(j < 16, 0.0, 1.0)], 1)
    # away from everything the positions cover and a last candidate one step back: the only descent behind the first bit
    last = line.copy()
    last[:, 0] += 40.0
    last[31, 0] = 69.5
    rows["last_only"] = last
    rows["quarter_steps"] = np.stack([0.25 * j, 0.5 * (j % 2)], 1)
    for nc in (2, 5, 31, 32):
        rows[f"line_nc{nc}"] = _row(line, nc)
        rows[f"fold_nc{nc}"] = _row(rows["fold"], nc)
    return rows


def lb_lattice_positions():
    """[n][2]: a quarter grid over and around the candidates (positions on a candidate, positions halfway between two), before
    the first candidate, beyond the last, and one idle position"""
    x, y = np.meshgrid(np.arange(-4.0, 36.01, 0.25), np.array([-2.0, -0.25, 0.0, 0.5, 1.0, 3.0]), indexing="ij")
    grid = np.stack([x.ravel(), y.ravel()], 1)
    return np.concatenate([grid, [[-3.0, 0.0], [40.0, 0.0], [np.nan, 0.0]]])


LB_NONFINITE = ((np.nan, 0.0), (np.inf, 0.0), (0.0, np.nan), (1e20, 0.0))  # the first: an idle position


def lb_nonfinite_positions(dtype):
    q = LB_NONFINITE if dtype == F32 else LB_NONFINITE[:3]  # 1e20: d^2 overflows in f32 only
    return np.array(q, dtype)


LB_REAL_N, LB_REAL_SIGMA, LB_REAL_SEED = 4096, 0.3, 71
LB_GAP = {F32: 1e-5, F64: 1e-13}  # one float distance carries about 2e-7 relative error: a bit is certain beyond 4e-7; 25 x that
LB_LEFT_OUT_MAX = 0.02


def lb_real_case(dtype):
    """(candidates, positions) in `dtype`: 32 candidates 0.25 apart on an arc of radius 12, positions scattered around them
    with sigma = 0.3"""
    rng = np.random.default_rng(LB_REAL_SEED)
    a = 0.25 * np.arange(LB_CAND) / 12.0
    cand = np.stack([12.0 * np.sin(a), 12.0 * (1.0 - np.cos(a))], 1)
    pos = cand[rng.integers(0, LB_CAND, LB_REAL_N)] + rng.normal(0.0, LB_REAL_SIGMA, (LB_REAL_N, 2))
    return cand.astype(dtype), pos.astype(dtype)


def lb_real_reference(dtype):
    """(candidates, positions, m, bad, compared[call]): `compared` is False where two consecutive candidate distances of the call
    differ by less than LB_GAP relative in f64 -- there a rounded distance may order them otherwise"""
    cand, pos = lb_real_case(dtype)
    m, bad, _, gap = lb_scan_reference(cand, pos)
    return cand, pos, m, bad, gap >= LB_GAP[dtype]


def lb_reach_table():
    """(table[n][4] = {leave, window, n_ref, c}, want[n]): the exactness argument stated by brute force -- every index p the
    workgroup's calls may have been entered at, 0 .. leave, keeps its window inside the candidates (or the path ends first),
    and the index stays below the window"""
    rows, want = [], []
    for W in (10, 20):
        for rem in (2, 20, 32, 33, 100):
            for c in (0, 7):
                for leave in range(41):
                    rows.append((leave, W, c + rem, c))
                    want.append(leave < W and all(min(p + W, rem) <= LB_CAND for p in range(leave + 1)))
    return np.array(rows, I32), np.array(want)


def lb_reach_reference(leave, W, n_ref, c):
    return bool(leave < W and all(min(p + W, n_ref - c) <= LB_CAND for p in range(leave + 1)))


def lb_tag_reference(seq):
    return (np.asarray(seq, np.uint64) & 0xFFFFFF) << 8


LB_EXCHANGE_B = (1, 2, 4, 5, 8, 9, 255, 256, 257, 511, 512)


def lb_exchange_words(B, tag, marks, seed=81):
    """(words[B], offset[B], badbit[B]): random offsets 0 .. 127 under `tag`, the bad bit at the workgroups `marks` names"""
    rng = np.random.default_rng(seed + B)
    off = rng.integers(0, 128, B)
    off[rng.integers(0, B)] = 127  # (the whole offset field somewhere)
    badbit = np.zeros(B, bool)
    badbit[[b for b in marks if 0 <= b < B]] = True
    return (np.uint64(tag) | (badbit * LB_BAD).astype(np.uint64) | off.astype(np.uint64)).astype(U32), off, badbit


def lb_exchange_marks(B):
    """{name: workgroups whose word carries the bad bit}"""
    rng = np.random.default_rng(82 + B)
    return {"none": [], "first": [0], "last_read": [B - 2], "last": [B - 1],
            "sparse": sorted(set(rng.integers(0, B, max(1, B // 40)).tolist()))}


def lb_exchange_reference(off, badbit, published):
    """(ok, E, bad) per workgroup: b waits for [0, b); it gives up where one of them never publishes"""
    B = off.size
    ok = np.array([published[:b].all() for b in range(B)])
    E = np.array([off[:b].max() if b and ok[b] else 0 for b in range(B)])
    bad = np.array([bool(badbit[:b].any()) and ok[b] for b in range(B)])
    return ok, E, bad


def lb_slots(fill=0):
    return np.full(LB_SLOT_WORDS, fill, U32)


def lb_published_everywhere(slots, words, published):
    """every copy of the returned buffer holds the words of the workgroups that published"""
    copies = slots.reshape(LB_COPIES, LB_COPY_STRIDE)[:, :words.size]
    return bool((copies[:, published] == words[None, published]).all())


# ------------------------------------------------------------------------------------------ sampler
KAT = (((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
        (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)))  # Random123's known-answer vectors (kat_vectors, philox4x32 10)


def oracle_philox(ctr, key):
    ctr, key = np.asarray(ctr, U32), np.asarray(key, U32)
    out = np.empty_like(ctr)
    for i in range(ctr.shape[0]):  # (the restatement takes one key per call)
        out[i] = [int(w) for w in philox.philox4x32_10(*ctr[i], key[i, 0], key[i, 1])]
    return out


def chol_f32():
    return philox.cholesky2(SIGMA).astype(F32)[[0, 1, 1], [0, 0, 1]]


def box_muller_words():
    """(ra, rb): each edge word for ra and rb, and for rb also the words nearest u = 1/4, 1/2, 3/4 and their neighbours"""
    quarter = [w for u in (0.25, 0.5, 0.75) for k in (-2, -1, 0, 1) for w in [((int(u * 2 ** 23) + k) << 9) & 0xFFFFFFFF]]
    rb = np.array(list(WORDS) + quarter + [w | 0x1FF for w in quarter], U32)
    ra, rb = np.meshgrid(np.array(WORDS, U32), rb, indexing="ij")
    return ra.ravel(), rb.ravel()


def box_muller_reference(ra, rb):
    ua, ub = philox.uniform_open(ra), philox.uniform_open(rb)
    rad, ang = np.sqrt(-2.0 * np.log(ua)), 2.0 * np.pi * ub
    L = philox.cholesky2(SIGMA).astype(F32).astype(F64)
    z0, z1 = rad * np.cos(ang), rad * np.sin(ang)
    return np.stack([L[0, 0] * z0, L[1, 0] * z0 + L[1, 1] * z1], axis=-1)


def box_muller_abs_err(P):
    ra, rb = box_muller_words()
    return np.abs(P.box_muller(ra, rb, chol_f32()).astype(F64) - box_muller_reference(ra, rb))
