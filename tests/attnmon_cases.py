"""Shared cases of the attention-monitor tests (tests/test_attnmon_cpu.py, tests/test_attnmon_gpu.py): synthetic sites
in svit_attn_fwd's operand convention, the measured error of exp2, and the comparison of ring entries and map rows with
the float64 yardstick `attnmon.attn_host` at the derived bar.

The bar, per probe row (attn_host evaluates it from the operands; nothing below comes from what the kernel gives):

  s_k   the kernel adds C = 96 + J products in fp32.  A product bf16 x bf16 has 16 significant bits and is exact in fp32,
        so only the C additions round, each within 2^-24 of a partial sum that is at most A_k = sum_j |q_j k_j|:
            |s^_k - s_k| <= C * 2^-24 * A_k
  d_k   one fp32 subtraction of lse2:  e_d = C * 2^-24 * A_k + 2^-24 * |d_k|
  p_k   p = 2^d, so an error e_d of d moves p by p * ln 2 * e_d to first order; the hardware's exp2 adds eps_exp relative
        and may flush a result below 2^-126 to zero, which adds at most 2^-126 absolute:
            e_p = p_k * (ln 2 * e_d + eps_exp) + 2^-126
  sums  to first order, and times 2 for the second-order terms and the fp64 summation (n * 2^-53, far below):
            sum_p   2 * sum_k e_p            m_cls  2 * e_p[0]          m_obj  2 * sum_{k > Lk} e_p
            pmax    2 * max_k e_p            H      2 * sum_k (|d_k| e_p + p_k e_d)       (H = - sum p d)
  an entry sums rows, so its bar is the sum of its rows' bars; min_H and sum_dev are fp32 casts of one row's value: the
  row's bar plus 2^-23 of the value.
eps_exp is not chosen here: it is 4 x the worst relative error of fp32 torch.exp2 on the device that runs the kernel,
against float64, over the very d values of the case (normal results only -- the flush term covers the rest), floored at
2^-23 (`measure_eps`).  Without a device the CPU tests take the floor itself.

Counts, first_bad, rows, row codes of bad rows and the header must match exactly.  The row the kernel names as the one
of least entropy must be a row whose host entropy lies within (its bar + the host minimum's bar) of the host minimum;
map rows are held per element at 2 * e_p, and the largest element of a map row must be a key whose host probability lies
within the pmax bar of the host's largest (a ring entry has no room for that key, so it is held where it can be read)."""
import math

import numpy as np
import torch

EPS_FLOOR = 2.0 ** -23


def measure_eps(d, device):
    """4 x the worst relative error of fp32 torch.exp2 on `device` over the float32 values d (results that are normal
    numbers), floored at 2^-23"""
    d32 = np.ascontiguousarray(d, dtype=np.float32).reshape(-1)
    d32 = d32[np.isfinite(d32) & (d32 > -126.0) & (d32 < 127.0)]
    if not len(d32):
        return EPS_FLOOR
    got = torch.exp2(torch.from_numpy(d32).to(device)).cpu().numpy().astype(np.float64)
    want = np.exp2(d32.astype(np.float64))
    return max(EPS_FLOOR, 4.0 * float(np.max(np.abs(got - want) / want)))


def bf16(a):
    """float array -> torch bf16 tensor (round to nearest even, as the pooling kernels store their operands)"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16)


def site(B, h, Lq, Lk, n_obj, DA, J, seed=26, sharp=1.0):
    """one synthetic site in the operand convention: qa[:, :96] ~ N(0, 0.35 sharp), qa[:, 96:96+J] ~ N(0, 0.5) (the bias
    terms), ka[:, :96] ~ N(0, 0.35), ka[:, 96:96+J] three ones (one-hot coordinates), columns past 96 + J zero; lse2 is the
    float64 log2-sum-exp2 of the bf16 operands' scores, rounded to fp32 -- what svit_attn_fwd would have saved, within
    its own error.  -> dict(qa, ka bf16 tensors, lse2 float32 array, geometry)"""
    rng = np.random.default_rng(seed)
    Nq, Nk = 1 + Lq + n_obj, 1 + Lk + n_obj
    Jd = J if J else DA - 96
    qa = np.zeros((B, h, Nq, DA), dtype=np.float32)
    ka = np.zeros((B, h, Nk, DA), dtype=np.float32)
    qa[..., :96] = rng.standard_normal((B, h, Nq, 96)) * 0.35 * sharp
    ka[..., :96] = rng.standard_normal((B, h, Nk, 96)) * 0.35
    qa[..., 96:96 + Jd] = rng.standard_normal((B, h, Nq, Jd)) * 0.5
    for c in range(3):
        hot = rng.integers(0, Jd, size=(B, h, Nk))
        np.put_along_axis(ka[..., 96:96 + Jd], hot[..., None], 1.0, axis=-1)
    qa, ka = bf16(qa), bf16(ka)
    s = np.einsum("bhqc,bhkc->bhqk", qa.float().numpy().astype(np.float64), ka.float().numpy().astype(np.float64))
    m = s.max(-1, keepdims=True)
    lse2 = (m[..., 0] + np.log2(np.exp2(s - m).sum(-1))).astype(np.float32)
    return dict(qa=qa, ka=ka, lse2=lse2, B=B, heads=h, Nq=Nq, Nk=Nk, DA=DA, bias_cols=J, Lq=Lq, Lk=Lk, n_obj=n_obj)


def host(s, kinds, K, eps_exp=EPS_FLOOR):
    from svit_amd import attnmon
    return attnmon.attn_host(s["qa"], s["ka"], s["lse2"], s["Lq"], s["Lk"], s["n_obj"], s["bias_cols"], kinds, K,
                             eps_exp=eps_exp)


def host_d(s, kinds, K):
    """the float32 d values of the site's probe rows: what exp2 is applied to"""
    return host(s, kinds, K)["per_row"]["d"]


def assert_entries(got, want, what=""):
    """ring entries of one site against attn_host's dict: every sum inside its bar, min_H / sum_dev inside theirs, the
    min-entropy row one the host could have named, everything else exactly"""
    e, bars = want["entries"], want["bars"]
    assert got.shape == e.shape, what
    for key in ("rows", "n_bad", "first_bad"):
        assert got[key].tobytes() == e[key].tobytes(), (what, key, got[key].tolist(), e[key].tolist())
    for key in ("sum_H", "sum_pmax", "sum_cls", "sum_obj", "sum_p", "sum_dev"):
        err = np.abs(got[key].astype(np.float64) - e[key].astype(np.float64))
        assert np.isfinite(bars[key]).all() and np.isfinite(e[key]).all(), (what, key)
        worst = int(np.argmax(err - bars[key]))
        assert (err <= bars[key]).all(), (what, key, worst, float(got[key][worst]), float(e[key][worst]),
                                          float(bars[key][worst]))
    per, code, gid = want["per_row"], want["code"], want["group"]
    G = int(gid.max()) + 1 if len(gid) else 1
    for i in range(len(e)):
        hd, g = divmod(i, G)
        if e["min_row"][i] < 0:
            assert got["min_row"][i] == -1 and got["min_H"][i] == 0.0, (what, i)
            continue
        sel = gid == g
        H, bH = per["H"][:, hd][:, sel], per["b_H"][:, hd][:, sel]
        good, cg = ~per["bad"][:, hd][:, sel], code[:, sel]
        at = np.argwhere((cg == got["min_row"][i]) & good)
        assert len(at) == 1, (what, i, "min_row names no good probe row", int(got["min_row"][i]))
        b, r = at[0]
        j = np.unravel_index(np.argmin(np.where(good, H, np.inf)), H.shape)
        assert H[b, r] - H[j] <= bH[b, r] + bH[j], (what, i, "min_row", float(H[b, r]), float(H[j]))
        assert abs(float(got["min_H"][i]) - H[b, r]) <= bH[b, r] + 2.0 ** -23 * abs(H[b, r]), (what, i, "min_H")


def assert_maps(got, want, samples, what=""):
    """map rows [samples, h, n_probe, Nk] against the host's P per element at 2 * e_p; bad rows carry no meaning"""
    P = want["P"][:samples]
    good = ~want["per_row"]["bad"][:samples]
    assert got.shape == P.shape, (what, got.shape, P.shape)
    bound = want["per_row"]["b_map"][:samples]
    err = np.abs(got.astype(np.float64) - P)
    assert (err[good] <= bound[good]).all(), (what, float(np.nanmax(err[good])))
    # the key of a row's peak (the ring has no room for it, a map has): one whose host value lies within the bar of the
    # host's largest
    Pg = np.where(good[..., None], P, 0.0)
    at = np.take_along_axis(Pg, got.argmax(-1)[..., None], -1)[..., 0]
    assert (Pg.max(-1) - at <= want["per_row"]["b_p"][:samples])[good].all(), (what, "argmax key")


def mutant(s, kinds, K, which):
    """the yardstick's entries with one mistake: "column" -- the last bias column dropped; "obj" -- the object mass
    started one key early; "ln" -- entropy with the natural log for log2"""
    from svit_amd import attnmon
    J = s["bias_cols"] if s["bias_cols"] else s["DA"] - 96
    if which == "column":
        return attnmon.attn_host(s["qa"], s["ka"], s["lse2"], s["Lq"], s["Lk"], s["n_obj"], J - 1, kinds, K)["entries"]
    if which == "obj":
        return _obj_early(s, kinds, K)
    e = host(s, kinds, K)["entries"].copy()
    e["sum_H"] *= math.log(2.0)
    return e


def _obj_early(s, kinds, K):
    h = host(s, kinds, K)
    e = h["entries"].copy()
    P, gid, bad = h["P"], h["group"], h["per_row"]["bad"]
    G = int(gid.max()) + 1
    early = np.nansum(np.where(bad[..., None], 0.0, P)[..., s["Lk"]:], axis=-1)         # k >= Lk instead of k > Lk
    for i in range(len(e)):
        hd, g = divmod(i, G)
        e["sum_obj"][i] = early[:, hd][:, gid == g].sum()
    return e
