"""Float64 references, a rounding-point emulation and a set of deliberately wrong variants ("mutants") of the NT
GEMM's epilogues (svit_gemm_nt, include/svit_hip.h), all on the CPU.

* reference(case)    float64, nothing rounded: what each epilogue IS.  The product is taken over the bf16 operands
                     (exact in float64), GELU and GELU' use float64 erf.
* emulate(case)      the same maths with the kernels' documented rounding points only: fp32 accumulation (an fp32
                     CPU matmul is the proxy), fp32 bias add, the epilogue in fp32 with the erf form that
                     common.h::gelu_parts documents (Abramowitz-Stegun 7.1.26, five terms), ONE bf16 rounding of
                     bf16 outputs, EPI_DGELU as an fp32 product with the bf16 aux rounded once.  Its distance from
                     the reference is the yardstick ("floor") of a case.
* MUTANTS            the float64 reference with ONE plausible kernel bug each (the `mutant=` argument of
                     reference); outputs the kernel stores as bf16 are rounded once, as the buggy kernel would.
* CASES, inputs      the shapes and epilogue variants of tests/test_gemm_parity_gpu.py and their deterministic
                     inputs; FORMS names the kernel forms and the shapes each of them takes.
* metric, case_bars  the per-element measure below and the bar (BAR_FACTOR x floor) of every output of a case.
                     tests/test_gemm_reference_cpu.py proves on the CPU that every applicable mutant lies at
                     >= 3 x bar; the GPU test applies the same bars to the kernels.

The measure, element by element
-------------------------------
h_ij = sum_k a_ik w_jk + bias_j is computed by the kernels in fp32, in an order that differs from tile form to tile
form.  Whatever the order, the computed value is h_ij + e_ij with |e_ij| <= (K + 1) u S_ij, u = 2^-24 and

    S_ij = sum_k |a_ik| |w_jk| + |bias_j|       (+ |old_ij| for accumulate; EPI_RESID: |aux_ij| + |s_i| times it,
                                                 s_i the row's scale -- a dropped sample, s = 0, is aux exactly)

(Higham, Accuracy and Stability of Numerical Algorithms, section 3.1; for random signs the error behaves like
sqrt(K) u S).  S_ij, not |h_ij| and not max |h|, is therefore the scale of the error a correct kernel can make in
element (i, j): where the terms cancel, |h_ij| is small and the permitted error is not.

fp32 outputs (EPI_RESID, EPI_F32):      m_ij = |got_ij - ref_ij| / S_ij.

bf16 outputs (EPI_BF16, EPI_GELU, EPI_DGELU) are out = bf16(f(h + e) + e_f), f the epilogue function and e_f the
error of its fp32 evaluation.  Rounding to bf16 (8 significant bits, round to nearest even) moves a value by at most
half a unit in the last place, which is at most 2^-8 |value|: the "one bf16 ulp of |ref|" allowance.  Hence

    |got - ref| <= 2^-8 |ref| + (1 + 2^-8) (|f'(xi)| |e| + |e_f|)

with xi between h and h + e.  The first term is what ONE rounding may cost and is taken off; what is left over
is compared with the scale of the second:

    m_ij = max(0, |got_ij - ref_ij| - 2^-8 |ref_ij|) / (S_ij D_ij + ABS_f / u)

    D_ij    the float64 derivative bound of the epilogue at h_ij over the interval the fp32 error can reach:
            1 for EPI_BF16, |aux_ij| for EPI_DGELU (out = acc * aux),
            |gelu'(h_ij)|  + C2 (K + 1) u S_ij for gelu(h),    C2 = max |gelu''|  = 2 pdf(0) < 1,
            |gelu''(h_ij)| + C3 (K + 1) u S_ij for gelu'(h),   C3 = max |gelu'''| < 1   (both bounds taken as 1)
    ABS_f   the absolute term: the largest distance of the emulated fp32 f (gelu_parts restated, with the one-ulp
            error HIP documents for __expf and the hardware reciprocal applied in either direction) from the
            float64 f over a dense grid on [-12, 12], beyond the fp32 rounding of the result itself.  It is what
            remains where |ref| falls below the approximation's error (gelu(-6) = -6e-9, the rational erf is good
            to 1.5e-7): there the relative allowance is worth nothing and S D alone would make the permitted error
            vanish.  Divided by u it enters the denominator in the units of the first term, so that one unit of m
            is "one fp32 rounding of S D, or one ABS_f".  0 for EPI_BF16 and EPI_DGELU.

Both m are dimensionless and of the order of sqrt(K) u for a correct kernel at every element, large or small; a
wrong value in one 4-column group of one row, or in the GELU tails, stands out by orders of magnitude wherever it is.
The floor of a case is max_ij m_ij of the emulation, and never less than u (no fp32 accumulation commits fewer than
one rounding of a partial sum of the size of S); bar = BAR_FACTOR x floor.  Neither ever sees a kernel's output.
"""
import functools
import math

import torch

from oracle import procedural as PR

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
U32 = 2.0 ** -24              # fp32 unit roundoff
BF16_ULP = 2.0 ** -8          # the largest relative move of one rounding to bf16
BAR_FACTOR = 3.0              # a margin over the emulation's own error, not a measurement
SENTINEL = 7.0                # what the GPU test pre-fills every output buffer with (exact in bf16)
ROW_SCALE = (1.0, 0.0, 1.6667, 0.75)      # cycled: neighbouring samples always differ
BIAS_AMP = 0.5
ROW_GAINS = (1.0, 0.5, 0.2, 1.0, 0.05, 0.7, 0.01, 0.35)     # per-row gain of the activations, cycled
H_STD = 3.0                   # std of a.w at gain 1: h covers [-6, 6] and beyond, the small gains crowd h around the bias
SMALL_X = 2.0 ** -5           # where the "no x.pdf" mutant drops the term
OLD_BAR_BF16, OLD_BAR_F32 = 1.5e-2, 1e-3   # the suite's present measure: max |got - ref| / max |ref|


# ------------------------------------------------------------------------------------------------- GELU ----
def _pdf(x):
    return torch.exp(-0.5 * x * x) * 0.3989422804014327


def gelu64(x):
    return x * 0.5 * (1.0 + torch.erf(x * 0.7071067811865476))


def dgelu64(x):
    return 0.5 * (1.0 + torch.erf(x * 0.7071067811865476)) + x * _pdf(x)


def d2gelu64(x):
    return _pdf(x) * (2.0 - x * x)


def gelu_tanh64(x):
    return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))


def gelu_parts32(x, pe=0.0, pt=0.0):
    """common.h::gelu_parts restated in fp32 torch: -> (gelu, gelu').  pe / pt in {-1, 0, 1} move exp and the
    reciprocal by one documented ulp (2^-22 of the value covers the argument scaling of __expf as well)."""
    assert x.dtype == F32
    ax = x.abs() * 0.70710678118654752
    e = torch.exp(-ax * ax) * (1.0 + pe * 2.0 ** -22)
    t = (1.0 / (1.0 + 0.3275911 * ax)) * (1.0 + pt * 2.0 ** -22)
    poly = t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429))))
    erf_abs = 1.0 - poly * e
    erfv = torch.where(x < 0, -erf_abs, erf_abs)
    cdf = 0.5 * (1.0 + erfv)
    pdf = 0.39894228040143268 * e
    assert cdf.dtype == F32
    return x * cdf, cdf + x * pdf


@functools.lru_cache(maxsize=None)
def abs_terms():
    """(ABS_gelu, ABS_dgelu): see the module docstring."""
    x = torch.linspace(-12.0, 12.0, (1 << 17) + 1, dtype=F32)
    x64 = x.to(F64)
    rg, rd = gelu64(x64), dgelu64(x64)
    ag = ad = 0.0
    for pe in (-1.0, 1.0):
        for pt in (-1.0, 1.0):
            g, d = gelu_parts32(x, pe, pt)
            ag = max(ag, float(((g.to(F64) - rg).abs() - 2.0 ** -22 * rg.abs()).clamp_min(0).max()))
            ad = max(ad, float(((d.to(F64) - rd).abs() - 2.0 ** -22 * rd.abs()).clamp_min(0).max()))
    return ag, ad


# ------------------------------------------------------------------------------------------------ cases ----
class Case:
    """one (shape, epilogue variant).  epi: bf16 | gelu | dgelu | resid | f32; save: EPI_GELU writes out2;
    rps: rows_per_sample (0 = no row_scale); inplace: out == aux; acc: accumulate; remap: (L, Ntok, off)."""

    def __init__(self, M, N, K, epi, save=True, rps=0, inplace=False, acc=False, remap=None):
        self.M, self.N, self.K, self.epi = M, N, K, epi
        self.save, self.rps, self.inplace, self.acc, self.remap = save, rps, inplace, acc, remap
        tag = epi
        if epi == "gelu" and not save:
            tag += "_nosave"
        if epi == "resid":
            tag += ("_rps%d" % rps if rps else "_noscale") + ("_inplace" if inplace else "")
        if epi == "f32":
            tag += ("_remap" if remap else "") + ("_acc" if acc else "")
        self.variant = tag
        self.name = "%dx%dx%d-%s" % (M, N, K, tag)

    @property
    def shape(self):
        return (self.M, self.N, self.K)

    @property
    def tensors(self):
        return ("out", "out2") if self.epi == "gelu" and self.save else ("out",)

    @property
    def out_bf16(self):
        return self.epi in ("bf16", "gelu", "dgelu")

    def __repr__(self):
        return "Case(%s)" % self.name


def remap_of(M):
    """(L, Ntok, off): M rows as M / L samples of L tokens, written behind one leading row of windows of L + 5."""
    L = M // 3 if M % 3 == 0 else (M // 2 if M % 2 == 0 else M)
    return (L, 1 + L + 4, 1)


def remap_rows(M, remap):
    L, ntok, off = remap
    r = torch.arange(M)
    return (r // L) * ntok + off + r % L


def remap_buffer_rows(M, remap):
    L, ntok, _ = remap
    return (M + L - 1) // L * ntok


def epilogue_list(M):
    """the whole epilogue list of a form.  The epilogue reads two scales and a boundary per wave ("rs_fast") when
    rows_per_sample >= 32 RB, one scale per row otherwise; a wave owns 32 RB rows, RB = FORMS[...]["rb"].  At M = 417:
      20   per-row on every tile;
      54   rs_fast on RB = 1 (sample boundaries inside 5 of its 14 wave blocks), per-row on RB = 2, 3, 5;
      139  boundaries at rows 139 and 278: rs_fast with a boundary inside two of the wave blocks on RB = 1 (of 14),
           RB = 2 (of 7) and RB = 3 (of 5); per-row on RB = 5;
      200  boundaries at rows 200 and 400 with three differing scales: rs_fast on every RB, and the only multi-sample
           one on RB = 5 (160-row wave blocks 160..319 and 320..416 each hold a boundary);
      M    one sample of scale 1.0: rs_fast with rs_lo == rs_hi, the same result as no scale at all."""
    out = [dict(epi="bf16"), dict(epi="gelu"), dict(epi="gelu", save=False), dict(epi="dgelu")]
    for rps in sorted({20, 54, 139, 200, M}):
        if rps <= M:
            out += [dict(epi="resid", rps=rps), dict(epi="resid", rps=rps, inplace=True)]
    out += [dict(epi="resid"), dict(epi="f32"), dict(epi="f32", acc=True),
            dict(epi="f32", remap=remap_of(M)), dict(epi="f32", remap=remap_of(M), acc=True)]
    return out


SMALL_LIST = [dict(epi="f32"), dict(epi="bf16")]

# kernel forms: name -> (cfg, stages, K-step; the svit_debug_set knobs 1, 0, 2), the N it accepts as that form (a
# forced tile that does not divide N silently becomes another tile) and whether it needs K % 64 == 0 (so does a
# ring kernel and a forced K-step of 64: otherwise the entry point runs another kernel); rb = 32-row blocks per wave
# of the tile (at MAIN_SHAPE for the heuristic, which takes the 128 x 96 K-step-64 tile there).  That a form's
# knobs select the kernel named here, at every shape form_shapes gives it, is checked: tests/test_gemm_nt_plan_cpu.py
# asks svit_debug_gemm_nt_plan -- the chooser the launch itself calls -- for family, tile, stages and K-step.
_RB = {0: 2, 2: 1, 4: 2, 5: 2, 6: 1, 7: 2, 9: 5, 10: 3}
FORMS = {"heuristic": dict(cfg=-1, stages=0, bk=0, n_small=96, k64=False)}
for _cfg, _n in ((0, 192), (2, 96), (4, 384)):
    for _st in (2, 3, 4):
        for _bk in (32, 64):
            FORMS["v2_cfg%d_s%d_bk%d" % (_cfg, _st, _bk)] = dict(cfg=_cfg, stages=_st, bk=_bk, n_small=_n, k64=_bk == 64)
for _cfg, _n in ((5, 192), (6, 96), (7, 384)):
    for _st in (2, 3, 4):
        FORMS["ring_cfg%d_s%d" % (_cfg, _st)] = dict(cfg=_cfg, stages=_st, bk=0, n_small=_n, k64=True)
FORMS["one_round_cfg9"] = dict(cfg=9, stages=0, bk=0, n_small=768, k64=False)       # 160 x 256: N % 256 == 0
FORMS["one_round_cfg10"] = dict(cfg=10, stages=0, bk=0, n_small=192, k64=False)     # 192 x 192: N % 192 == 0

MAIN_SHAPE = (417, 768, 448)      # partial last tile for 128-, 160- and 192-row tiles and a partial 16-row slab; N
                                  # divides by 96, 128, 192 and 256; K % 64 == 0 and the heuristic's K-step-64 shortcut
HEURISTIC_SHAPES = [(417, 384, 96), (130, 384, 2304)]      # K % 64 != 0; the long-K choice (4 stages)


def form_shapes(form):
    """[(shape, epilogue list)] of a form: the whole list at M = 417, EPI_F32 and EPI_BF16 at the small shapes
    (K = 32 and 64: one K-step under a 2- to 4-stage prologue, nk = 1 < STAGES on the ring; M = 1 and 15)."""
    f = FORMS[form]
    out = [(MAIN_SHAPE, epilogue_list(MAIN_SHAPE[0]))]
    if form == "heuristic":
        out += [(s, epilogue_list(s[0])) for s in HEURISTIC_SHAPES]
    for K in ((64,) if f["k64"] else (32, 64)):
        for M in (1, 15, 130):
            out.append(((M, f["n_small"], K), SMALL_LIST))
    return out


def _all_cases():
    seen, out = set(), []
    for form in FORMS:
        for shape, lst in form_shapes(form):
            for kw in lst:
                c = Case(*shape, **kw)
                if c.name not in seen:
                    seen.add(c.name)
                    out.append(c)
    return out


for _f in FORMS.values():
    _f["rb"] = _RB.get(_f["cfg"], 1)

CASES = _all_cases()
CASE_BY_NAME = {c.name: c for c in CASES}


def case_of(shape, kw):
    return CASE_BY_NAME[Case(*shape, **kw).name]


# ----------------------------------------------------------------------------------------------- inputs ----
@functools.lru_cache(maxsize=8)
def inputs(M, N, K):
    """deterministic operands of a shape, shared by all its epilogue variants: a, w bf16; bias f32 [N]; aux32 f32
    [M, N] (residual); auxbf bf16 [M, N] (saved gelu'); old f32 [M, N] (accumulate); pad_cols [M, 8] (what lies
    beside aux in a wider buffer)."""
    tag = "%d_%d_%d" % (M, N, K)
    gains = torch.tensor([ROW_GAINS[i % len(ROW_GAINS)] for i in range(M)], dtype=F32)
    a = (PR.tensor("gp:a" + tag, (M, K), 1.0) * gains[:, None]).to(BF16)
    w = PR.tensor("gp:w" + tag, (N, K), 3.0 * H_STD / math.sqrt(K)).to(BF16)     # uniform [-1, 1): variance 1/3 each
    return dict(a=a, w=w,
                bias=PR.tensor("gp:b" + tag, (N,), BIAS_AMP),
                aux32=PR.tensor("gp:r" + tag, (M, N), 1.0),
                auxbf=PR.tensor("gp:d" + tag, (M, N), 1.1).to(BF16),
                old=PR.tensor("gp:o" + tag, (M, N), 2.0),
                pad_cols=PR.tensor("gp:p" + tag, (M, 8), 1.0, center=3.0))


def row_scale_of(case):
    n = (case.M + case.rps - 1) // case.rps
    return torch.tensor([ROW_SCALE[i % len(ROW_SCALE)] for i in range(n)], dtype=F32)


def aux_buffer(case, pad):
    """the [M, N + pad] buffer whose first N columns are the case's aux (f32 residual or bf16 saved gelu')."""
    x = inputs(*case.shape)
    aux = x["aux32"] if case.epi == "resid" else x["auxbf"]
    return torch.cat([aux, x["pad_cols"][:, :pad].to(aux.dtype)], 1)


def old_buffer(case):
    """what the output buffer of an accumulate case holds before the call: `old` at the rows the call writes,
    the sentinel elsewhere (rows outside the remap window)."""
    old = inputs(*case.shape)["old"]
    if not case.remap:
        return old.clone()
    buf = torch.full((remap_buffer_rows(case.M, case.remap), case.N), SENTINEL, dtype=F32)
    buf[remap_rows(case.M, case.remap)] = old
    return buf


# ------------------------------------------------------------------------------- reference and mutants ----
MUTANTS = ("drop_kstep", "stale_slab", "bias_shift4", "bias_dup8", "bias_missing_out2", "gelu_tanh",
           "dgelu_no_xpdf", "dgelu_at_bf16_h", "double_round", "rs_first_row", "rs_boundary_off1", "rs_div_plus1",
           "rs_on_residual", "acc_unremapped", "aux_ld_n", "swap_halves_last_tile")
AUX_PAD = 4                   # the width beyond N of the aux buffer the aux_ld_n mutant mis-reads
NO_EXCEPTIONS = ()            # mutants that could not be lifted to 3 x bar: none (the issue allows two)


def mutant_applies(name, case):
    M, N, K, epi = case.M, case.N, case.K, case.epi
    if name == "stale_slab":                       # the last PARTIAL 16-row slab takes the previous slab's accumulators
        return M % 16 != 0 and M > 16
    if name in ("bias_shift4", "bias_dup8"):
        return epi != "dgelu"                      # (EPI_DGELU takes no bias)
    if name in ("bias_missing_out2", "dgelu_no_xpdf", "dgelu_at_bf16_h"):
        return epi == "gelu" and case.save
    if name == "gelu_tanh":
        return epi == "gelu"
    if name == "double_round":
        return epi in ("bf16", "dgelu")
    if name in ("rs_first_row", "rs_boundary_off1", "rs_div_plus1"):
        return epi == "resid" and 0 < case.rps < M
    if name == "rs_on_residual":                   # (a single sample has scale 1.0: nothing to see)
        return epi == "resid" and 0 < case.rps < M
    if name == "acc_unremapped":
        return epi == "f32" and case.acc and case.remap is not None
    if name == "aux_ld_n":
        return epi in ("resid", "dgelu") and M > 1
    return True


def _b16(x):
    return x.to(F32).to(BF16).to(F64)


def terms(case):
    """float64 (acc, bias [N] or None, S [M, N]) of a case; S as in the module docstring."""
    x = inputs(*case.shape)
    A, W = x["a"].to(F64), x["w"].to(F64)
    acc = A @ W.t()
    S = A.abs() @ W.abs().t()
    bias = None
    if case.epi != "dgelu":
        bias = x["bias"].to(F64)
        S = S + bias.abs()
    if case.epi == "resid":
        if case.rps:
            S = S * row_scale_of(case).to(F64).abs()[torch.arange(case.M) // case.rps][:, None]
        S = S + x["aux32"].to(F64).abs()
    if case.acc:
        S = S + x["old"].to(F64).abs()
    return acc, bias, S


def reference(case, mutant=None):
    """-> {"out": [M, N] float64 (logical rows: a remap only says where they are stored), "out2": ...}."""
    assert mutant is None or (mutant in MUTANTS and mutant_applies(mutant, case)), (mutant, case)
    M, N, K, epi = case.M, case.N, case.K, case.epi
    x = inputs(M, N, K)
    acc, bias, _ = terms(case)
    if mutant == "drop_kstep":                     # the last 32-wide K-step, one 16-row slab of the last row tile
        r0 = (M - 1) // 128 * 128
        if case.rps:                               # (a slab of a dropped sample, scale 0, shows nothing of the product:
            rs = row_scale_of(case)                # the first slab of the tile that begins in a kept sample)
            r0 = next(r for r in range(r0, M, 16) if float(rs[r // case.rps]) != 0.0)
        r1 = min(r0 + 16, M)
        acc = acc.clone()
        acc[r0:r1] -= x["a"][r0:r1, K - 32:].to(F64) @ x["w"][:, K - 32:].to(F64).t()
    if mutant == "stale_slab":
        s0 = M // 16 * 16
        acc = acc.clone()
        acc[s0:] = acc[s0 - 16:s0 - 16 + (M - s0)]
    b = torch.zeros(N, dtype=F64) if bias is None else bias.clone()
    if mutant == "bias_shift4":                    # one 4-column group reads the group to its left
        c0 = 4 * max((N // 4) // 2, 1)
        b[c0:c0 + 4] = bias[c0 - 4:c0]
    if mutant == "bias_dup8":                      # the second float4 of one 8-column group = the first
        g = 8 * ((N // 8) // 2)
        b[g + 4:g + 8] = bias[g:g + 4]
    h = acc + b
    out = {}
    if epi == "bf16":
        out["out"] = _b16(acc) + b if mutant == "double_round" else h
    elif epi == "gelu":
        out["out"] = gelu_tanh64(h) if mutant == "gelu_tanh" else gelu64(h)
        if case.save:
            h2 = acc if mutant == "bias_missing_out2" else h
            if mutant == "dgelu_at_bf16_h":
                h2 = _b16(h2)
            d = dgelu64(h2)
            if mutant == "dgelu_no_xpdf":          # a "small x" shortcut: cdf alone
                small = h2.abs() < SMALL_X
                d = torch.where(small, d - h2 * _pdf(h2), d)
            out["out2"] = d
    elif epi == "dgelu":
        aux = x["auxbf"].to(F64)
        if mutant == "aux_ld_n":
            aux = aux_buffer(case, AUX_PAD).to(F64).flatten()[:M * N].reshape(M, N)
        out["out"] = (_b16(acc) if mutant == "double_round" else acc) * aux
    elif epi == "resid":
        aux = x["aux32"].to(F64)
        if mutant == "aux_ld_n":
            aux = aux_buffer(case, AUX_PAD).to(F64).flatten()[:M * N].reshape(M, N)
        s = torch.ones(M, dtype=F64)
        if case.rps:
            rs = row_scale_of(case).to(F64)
            r = torch.arange(M)
            idx = r // case.rps
            if mutant == "rs_first_row":           # the scale of the first row of a 32-row wave block for all of it
                idx = (r // 32 * 32) // case.rps
            if mutant == "rs_boundary_off1":
                idx = (r - 1).clamp_min(0) // case.rps
            if mutant == "rs_div_plus1":
                idx = r // (case.rps + 1)
            s = rs[idx]
        out["out"] = s[:, None] * (aux + h) if mutant == "rs_on_residual" else aux + s[:, None] * h
    else:
        o = h
        if case.acc:
            old = x["old"].to(F64)
            if mutant == "acc_unremapped":
                old = old_buffer(case).to(F64)[:M]
            o = o + old
        out["out"] = o
    if mutant == "swap_halves_last_tile":          # columns 4..7 of every 8-column store <-> 0..3, last 96 columns only
        for t in out:
            o = out[t].clone()
            o[:, N - 96:] = out[t][:, N - 96:].reshape(M, 12, 2, 4).flip(2).reshape(M, 96)
            out[t] = o
    if mutant is not None and case.out_bf16:
        out = {t: _b16(v) for t, v in out.items()}
    return out


def emulate(case):
    """the kernels' documented rounding points: -> {"out", "out2"} as float64 copies of what would be stored."""
    M, N, K, epi = case.M, case.N, case.K, case.epi
    x = inputs(M, N, K)
    acc = x["a"].to(F32) @ x["w"].to(F32).t()
    v = acc if epi == "dgelu" else acc + x["bias"]
    out = {}
    if epi == "bf16":
        out["out"] = v.to(BF16)
    elif epi == "gelu":
        g, d = gelu_parts32(v)
        out["out"] = g.to(BF16)
        if case.save:
            out["out2"] = d.to(BF16)
    elif epi == "dgelu":
        out["out"] = (v * x["auxbf"].to(F32)).to(BF16)
    elif epi == "resid":
        s = torch.ones(M, dtype=F32)
        if case.rps:
            s = row_scale_of(case)[torch.arange(M) // case.rps]
        out["out"] = x["aux32"] + s[:, None] * v
    else:
        out["out"] = v + x["old"] if case.acc else v
    assert all(o.dtype == (BF16 if case.out_bf16 else F32) for o in out.values())
    return {t: o.to(F64) for t, o in out.items()}


# ----------------------------------------------------------------------------------------------- metric ----
@functools.lru_cache(maxsize=None)
def _yardstick(name):
    """(reference outputs, {tensor: (allowance factor, denominator [M, N])}) of a case."""
    case = CASE_BY_NAME[name]
    ref = reference(case)
    acc, bias, S = terms(case)
    K = case.K
    den = {}
    if not case.out_bf16:
        den["out"] = S
    elif case.epi == "bf16":
        den["out"] = S
    elif case.epi == "dgelu":
        den["out"] = S * inputs(*case.shape)["auxbf"].to(F64).abs()
    else:
        h = acc + bias
        ag, ad = abs_terms()
        reach = (K + 1) * U32 * S
        den["out"] = S * (dgelu64(h).abs() + reach) + ag / U32
        if case.save:
            den["out2"] = S * (d2gelu64(h).abs() + reach) + ad / U32
    return ref, den


def metric(case, tensor, got):
    """max_ij m_ij of `got` [M, N] (anything convertible to float64) -> (value, (row, col) of the worst element)."""
    ref, den = _yardstick(case.name)
    r = ref[tensor]
    err = (got.to(F64) - r).abs()
    if case.out_bf16:
        err = (err - BF16_ULP * r.abs()).clamp_min(0)
    m = err / (den[tensor] + 1e-300)
    i = int(m.argmax())
    return float(m.flatten()[i]), divmod(i, case.N)


def old_measure(got, ref):
    """the suite's present measure: max |got - ref| / max |ref| over the whole tensor."""
    return float((got.to(F64) - ref).abs().max() / (ref.abs().max() + 1e-12))


@functools.lru_cache(maxsize=None)
def case_floors(name):
    case = CASE_BY_NAME[name]
    emu = emulate(case)
    return {t: max(metric(case, t, emu[t])[0], U32) for t in case.tensors}


def case_bars(name):
    return {t: BAR_FACTOR * f for t, f in case_floors(name).items()}
