"""Shared cases of the activation-monitor tests (tests/test_actmon_cpu.py, tests/test_actmon_gpu.py): the synthetic
sites, the bad rows placed in them, three mutants of the yardstick and the comparison of ring entries with the float64
yardstick at the derived bar."""
import numpy as np

# a site has at most 2^24 rows (more is refused).  Either side sums its terms within n * 2^-53 <= 2^-29 of sum |term| in
# any order, and a kernel term is within 2^-40 of the yardstick's: together below 2^-28 + 2^-40 < 2^-27 of sum |term|
BAR = 2.0 ** -27

SIZES = ("1", "3", "W - 1", "W", "W + 1", "3 W + 5")


def rows_of(size, W):
    return {"1": 1, "3": 3, "W - 1": W - 1, "W": W, "W + 1": W + 1, "3 W + 5": 3 * W + 5}[size]


def sites(W, seed=24):
    """-> (list of [a, b] float32 arrays, b None for an lse site; where: name -> index).  Both kinds at 1, 3, W - 1, W,
    W + 1 and 3 W + 5 rows; plain finite values: mean ~ N(0, 0.3), rstd log-normal, lse ~ N(5, 3) (some negative)"""
    rng = np.random.default_rng(seed)
    out, where = [], {}
    for size in SIZES:
        n = rows_of(size, W)
        where["ln " + size] = len(out)
        out.append([(rng.standard_normal(n) * 0.3).astype(np.float32),
                    np.exp(rng.standard_normal(n) * 0.5).astype(np.float32)])
        where["lse " + size] = len(out)
        out.append([(5.0 + 3.0 * rng.standard_normal(n)).astype(np.float32), None])
    return out, where


def ties(s, where):
    """the extremum twice in one site, in two windows' reach: the smaller row wins -> {site: arg}"""
    ln, lse = s[where["ln W"]], s[where["lse W - 1"]]
    ln[1][[100, 3000]] = np.float32(ln[1].min() * 0.5)
    lse[0][[7, 4000]] = np.float32(lse[0].max() + 1.0)
    return {where["ln W"]: 100, where["lse W - 1"]: 7}


def bad_rows(s, where, W):
    """bad rows on a site's first and last row, on either side of a window edge, in two windows at once, and two sites
    without a good row -> {site: (n_bad, first_bad)}"""
    a, b = s[where["ln 3 W + 5"]]
    a[0] = np.nan                       # (its rstd stays finite: the "summed as zero-mean" mutant counts it)
    a[W - 1] = -np.inf
    b[W] = 0.0
    b[3 * W + 4] = np.inf
    a, _ = s[where["lse 3 W + 5"]]
    a[W - 1], a[W], a[3 * W + 4] = np.nan, np.inf, -np.inf
    a, b = s[where["ln W + 1"]]
    a[0] = np.nan
    b[W] = -1.5
    a, b = s[where["ln 3"]]
    a[0], b[1], b[2] = np.inf, np.nan, -0.0
    s[where["lse 1"]][0][0] = np.nan
    return {where["ln 3 W + 5"]: (4, 0), where["lse 3 W + 5"]: (3, W - 1), where["ln W + 1"]: (2, 0),
            where["ln 3"]: (3, 0), where["lse 1"]: (1, 0)}


def mutant_sums(s, which, W):
    """the yardstick's sums with one mistake: "rstd" -- 1 / rstd for 1 / rstd^2; "zero_mean" -- a bad row whose rstd is
    usable summed with mean 0 instead of left out; "window" -- the second window of every site dropped"""
    from svit_amd import actmon
    out = np.zeros(len(s))
    np_err = np.seterr(all="ignore")        # (the values masked out below are computed first)
    try:
        _mutant_sums(s, which, W, out, actmon)
    finally:
        np.seterr(**np_err)
    return out


def _mutant_sums(s, which, W, out, actmon):
    for i, (a, b) in enumerate(s):
        bad = actmon.bad_rows(a, b)
        a64 = a.astype(np.float64)
        if b is None:
            term = np.where(bad, 0.0, a64)
        else:
            b64 = np.where(actmon.bad_rows(b), 1.0, b.astype(np.float64))       # (rstd itself unusable: never a term)
            inv = 1.0 / b64 if which == "rstd" else 1.0 / (b64 * b64)
            term = np.where(bad, 0.0, np.where(bad, 0.0, a64) ** 2 + inv)
            if which == "zero_mean":
                usable = bad & ~actmon.bad_rows(b) & ~(b <= 0)
                term = np.where(usable, inv, term)
        if which == "window":
            term[W:2 * W] = 0.0
        out[i] = term.sum()
    return out


def assert_entries(got, want, mass, what=""):
    """ring entries against acts_host's: the sum inside BAR * sum |term|, everything else exactly"""
    assert got.shape == want.shape
    assert np.isfinite(want["sum"]).all() and np.isfinite(mass).all(), what
    err = np.abs(got["sum"] - want["sum"])
    worst = int(np.argmax(err - BAR * mass))
    assert (err <= BAR * mass).all(), (what, "sum", worst, float(got["sum"][worst]), float(want["sum"][worst]))
    for key in ("ext", "ext2", "arg", "n_bad", "first_bad", "rows"):
        assert got[key].tobytes() == want[key].tobytes(), (what, key, np.flatnonzero(got[key] != want[key])[:8],
                                                           got[key][got[key] != want[key]][:8],
                                                           want[key][got[key] != want[key]][:8])
