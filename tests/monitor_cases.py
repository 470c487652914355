"""Shared cases of the tensor-monitor tests (tests/test_monitor_cpu.py, tests/test_monitor_gpu.py): the synthetic
buffer and its made-up tensor table, the special values placed in it, and the comparison of a ring row with the float64
yardstick at the derived bar."""
import numpy as np

# both sides sum at most 2^22 non-negative fp64 terms per tensor: in any order the relative error is at most
# n * 2^-53 <= 2^-31 each, so they differ by at most 2^-30 of the value
BAR = 2.0 ** -30


def layout(W):
    """-> (table int64 [80, 2], n, where): tensors of sizes 1, 3, 4, 96, then 70 of 4 elements inside window 0, an
    8-element gap (never counted), W - 1, one that ends exactly on the window edge 2 W, W (from edge to edge), W + 1,
    3 W + 5 and a last one that ends at n with n % 4 == 1.  Every begin is a multiple of 4.  `where` names the rows."""
    rows, where, cur = [], {}, 0

    def put(name, size):
        nonlocal cur
        where[name] = len(rows)
        rows.append([cur, cur + size])
        cur = (cur + size + 3) // 4 * 4

    for s in (1, 3, 4, 96):
        put("size %d" % s, s)
    for i in range(70):
        put("small %d" % i, 4)
    where["gap"] = (cur, cur + 8)
    cur += 8
    put("W - 1", W - 1)
    assert cur < 2 * W
    put("to the edge", 2 * W - cur)
    assert cur == 2 * W
    put("W", W)
    put("W + 1", W + 1)
    put("3 W + 5", 3 * W + 5)
    put("last", 1001)
    n = rows[-1][1]
    assert n % 4 == 1 and rows[where["small 69"]][1] < W and len(rows) == 80
    return np.ascontiguousarray(np.array(rows, dtype=np.int64)), n, where


def buffers(n, seed=23):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * 0.01).astype(np.float32), (rng.standard_normal(n) * 0.05).astype(np.float32)


def poison_gap(g, p, where):
    a, b = where["gap"]
    g[a:b] = np.nan
    p[a:b] = np.nan


DENORMAL = np.float32(1e-41)


def special_values(g, table, where, W):
    """NaN, +inf, -inf, 1e30 and a denormal inside tensors -> {row: (n_bad, first_bad)} of the rows that hold a
    non-finite element.  -inf on the last element of "to the edge" (left of the window edge 2 W), NaN on the first of
    "W" (right of it), two NaN in "W + 1" -- offset 100 and its last element, which lies in the next window -- and +inf
    on the last element of "3 W + 5"."""
    t = {k: table[v] for k, v in where.items() if k != "gap"}
    g[t["size 96"][0] + 17] = 1e30                      # finite: its square overflows fp32, not fp64
    g[t["size 3"][0] + 1] = DENORMAL
    g[t["to the edge"][1] - 1] = -np.inf
    g[t["W"][0]] = np.nan
    g[t["W + 1"][0] + 100] = np.nan
    g[t["W + 1"][1] - 1] = np.nan
    g[t["3 W + 5"][1] - 1] = np.inf
    assert t["to the edge"][1] == t["W"][0] == 2 * W
    return {where["to the edge"]: (1, int(t["to the edge"][1] - t["to the edge"][0] - 1)), where["W"]: (1, 0),
            where["W + 1"]: (2, 100), where["3 W + 5"]: (1, 3 * W + 4)}


def assert_entries(got, want, what=""):
    """a ring row's entries against stats_host's: both sums of squares inside BAR, everything else exactly"""
    assert got.shape == want.shape
    for key in ("sumsq_g", "sumsq_p"):
        k, h = got[key], want[key]
        assert np.isfinite(h).all(), (what, key)
        err = np.abs(k - h)
        worst = int(np.argmax(err - BAR * h))
        assert (err <= BAR * h).all(), (what, key, worst, float(k[worst]), float(h[worst]))
    for key in ("absmax_g", "n_bad", "first_bad", "reserved"):
        assert got[key].tobytes() == want[key].tobytes(), (what, key, np.flatnonzero(got[key] != want[key])[:8])
