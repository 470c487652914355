"""Shared cases of the update-monitor tests (tests/test_updmon_cpu.py, tests/test_updmon_gpu.py): the weights before and
after a known perturbation on the synthetic buffer of tests/monitor_cases.py, the float32 AdamW step of the stall check
and the comparison of a ring row with the float64 yardstick at the derived bar."""
import numpy as np

from tests import monitor_cases as M

# Delta is one IEEE subtraction on both sides.  Either side sums at most 2^22 fp64 terms per tensor: in any order each sum
# is within 2^22 * 2^-53 = 2^-31 of sum |term| of the exact one, so they differ by at most 2^-30 of it; the device may fuse
# a product into the following addition (2^-53 relative per term), which the factor two absorbs.
BAR = 2.0 ** -29
SUMS = ("sumsq_d", "sumsq_p", "dot_dg", "sumsq_g", "sumsq_m", "sum_v")
EXACT = ("absmax_d", "n_still", "n_one_ulp", "reserved")


def from_key(k):
    """the inverse of updmon.ulp_key: int64 keys -> float32"""
    i = np.asarray(k, dtype=np.int64).astype(np.int32)
    return (i ^ ((i >> 31) & np.int32(0x7fffffff))).view(np.float32)


def neighbour(x, up=True):
    """the adjacent float32 above (below) each element, by the key"""
    from svit_amd import updmon
    return from_key(updmon.ulp_key(x) + (1 if up else -1))


def neighbour1(x, up=True):
    """neighbour() of one number -> numpy.float32"""
    return neighbour(np.array([x], dtype=np.float32), up)[0]


def buffers(n, seed=31):
    """(p_old, g, m, v) float32 [n]: weights of 0.05, gradients of 0.01, moments of their sizes (v non-negative)"""
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal(n) * 0.05).astype(np.float32)
    g = (rng.standard_normal(n) * 0.01).astype(np.float32)
    m = (rng.standard_normal(n) * 0.01).astype(np.float32)
    v = (rng.standard_normal(n) ** 2 * 1e-4).astype(np.float32)
    return p, g, m, v


def perturb(p_old, table, where, W, seed=37):
    """p_old (changed in a few places, in place) -> (p_new, expect).  About a fifth of the elements keep their bits, a
    fifth move to an adjacent float, the rest step by about 1e-3 relative.  Placed by hand: "small 0" does not move at
    all and "small 1" moves one ulp everywhere; +0.0 -> -0.0 in "size 4"; in "size 96" one element crosses the binade
    edge at 1.0 by one ulp, one goes from 0.99 to 1.01, one denormal moves to the next; an unchanged element on either
    side of the window edges W and 2 W with changed neighbours; the first and the last element of "W + 1" and the very
    last element of the buffer unchanged.  expect: {row: (n_still, n_one_ulp)} of the tensors laid out by hand."""
    rng = np.random.default_rng(seed)
    n = len(p_old)
    t = {k: table[v] for k, v in where.items() if k != "gap"}
    p_old[p_old == 0] = np.float32(0.05)                # (none in practice: a zero moves nowhere by a relative step)
    a96 = int(t["size 96"][0])
    p_old[a96 + 3] = neighbour1(1.0, up=False)       # 0x3f7fffff
    p_old[a96 + 4] = np.float32(0.99)
    p_old[a96 + 5] = M.DENORMAL
    a4 = int(t["size 4"][0])
    p_old[a4 + 2] = np.float32(0.0)
    kind = rng.random(n)
    p_new = (p_old * (1 + 1e-3 * (1 + rng.random(n))).astype(np.float32)).astype(np.float32)
    assert (p_new.view(np.int32) != p_old.view(np.int32))[p_old != 0].all()
    one = (kind >= 0.2) & (kind < 0.4)
    p_new[one] = neighbour(p_old[one], up=True)
    still = kind < 0.2
    p_new[still] = p_old[still]
    far = p_old * np.float32(1.002)

    def set_still(i, neighbours=()):
        p_new[i] = p_old[i]
        for j in neighbours:
            p_new[j] = far[j]

    for edge in (W, 2 * W):
        set_still(edge - 1, (edge - 2,))
        set_still(edge, (edge + 1,))
    a, b = (int(x) for x in t["W + 1"])
    set_still(a, (a + 1,))
    set_still(b - 1, (b - 2,))
    set_still(n - 1, (n - 2,))
    a, b = (int(x) for x in t["small 0"])
    p_new[a:b] = p_old[a:b]
    a, b = (int(x) for x in t["small 1"])
    p_new[a:b] = neighbour(p_old[a:b], up=False)
    p_new[a4:a4 + 4] = far[a4:a4 + 4]
    p_new[a4 + 2] = np.float32(-0.0)
    p_new[a96:a96 + 96] = far[a96:a96 + 96]
    p_new[a96 + 3] = np.float32(1.0)
    p_new[a96 + 4] = np.float32(1.01)
    p_new[a96 + 5] = neighbour1(M.DENORMAL, up=True)
    expect = {where["small 0"]: (4, 0), where["small 1"]: (0, 4), where["size 4"]: (0, 1), where["size 96"]: (0, 2)}
    return p_new, expect


def adamw_first_step(p, g, lr, wd=0.0, betas=(0.9, 0.999), eps=1e-8):
    """one AdamW step from zero moments in NumPy float32, each operation rounded once -> (p_new, m, v)"""
    f = np.float32
    p, g = np.asarray(p, dtype=f), np.asarray(g, dtype=f)
    b1, b2 = f(betas[0]), f(betas[1])
    m = g * (f(1) - b1)
    v = (g * g) * (f(1) - b2)
    bc1, bc2 = f(1) - b1, np.sqrt(f(1) - b2)
    pw = p * (f(1) - f(lr) * f(wd))
    denom = np.sqrt(v) / bc2 + f(eps)
    return (pw - (f(lr) / bc1) * (m / denom)).astype(f), m, v


def assert_row(got, want, terms, what="", head=True):
    """a ring row against update_host's: the six sums inside BAR * sum |term| (`terms`: updmon.abs_terms_host), everything
    else -- the header included -- exactly"""
    if head:
        assert got["head"].tobytes() == want["head"].tobytes(), (what, got["head"], want["head"])
    g, w = got["entry"], want["entry"]
    assert g.shape == w.shape == terms.shape
    for key in SUMS:
        k, h, s = g[key], w[key], terms[key]
        assert np.isfinite(h).all() and np.isfinite(s).all(), (what, key)
        err = np.abs(k - h)
        worst = int(np.argmax(err - BAR * s))
        assert (err <= BAR * s).all(), (what, key, worst, float(k[worst]), float(h[worst]), float(s[worst]))
    for key in EXACT:
        assert g[key].tobytes() == w[key].tobytes(), (what, key, np.flatnonzero(g[key] != w[key])[:8])


def worst_excess(got, want, terms):
    """the largest |got - want| / (BAR * sum |term|) over the six sums and the tensors: above 1 misses the bar"""
    worst = 0.0
    for key in SUMS:
        s = terms[key]
        err = np.abs(got["entry"][key] - want["entry"][key])
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(s > 0, err / (BAR * s), np.where(err > 0, np.inf, 0.0))
        worst = max(worst, float(r.max()))
    return worst
