"""Dense references, a rounding-point emulation and a set of deliberately wrong variants ("mutants") of the
fused pooled attention (svit_attn_fwd / svit_attn_bwd, include/svit_hip.h), all on the CPU.

Operand convention (the header's): `qa . ka^T` IS the score in the log2 domain; the residual `qa[..., :96]` is
added to every query row but row 0; `dk` is taken with respect to the UN-scaled pooled keys
(dk = scale * sum_q P (dP - delta) q) and `dqa` with respect to `qa` (hence a factor ln 2).

* reference_fwd / reference_bwd   float64, nothing rounded: what the operation IS ([B, h, ...]; *_2d = one slice).
* emulate_fwd_2d / emulate_bwd_2d the same maths, dense and untiled, with the kernels' documented rounding points
                                  only: bf16 operands, fp32 scores, P (and dS) rounded to bf16 before the second
                                  product, the row sum taken over the ROUNDED P (the kernels sum it on the matrix
                                  pipe from the bf16 fragment), fp32 accumulation, `attention / l` rounded to bf16
                                  and then once more after the residual add, bf16 dqa, delta from the bf16 ctx.
                                  Its distance from the reference is the yardstick ("floor") of a case.
* FWD_MUTANTS / BWD_MUTANTS       the float64 reference with ONE plausible kernel bug each (the `mutant=` argument
                                  of reference_fwd_2d / reference_bwd_2d).
* rel_max                         max |got - ref| / max |ref|, applied per tensor to the ATTENTION-ONLY part
                                  (ctx - residual) and to each section of dqa separately.
* CASES, make_inputs, case_bars   the shapes of tests/test_attention_parity_gpu.py, their deterministic inputs
                                  (two families: flat and peaked scores) and the bars (3 x floor) of every tensor.
                                  tests/test_attention_reference_cpu.py proves on the CPU that every applicable
                                  mutant lies at >= 3 x bar; the GPU test applies the same bars to the kernels.

Everything here works on one (batch, head) slice at a time (2-D tensors); the [B, h, ...] wrappers loop, so the
memory of a float64 reference stays bounded at the step's own grids."""
import functools
import math

import torch

from oracle import procedural as PR

HD = 96                      # head dim of q.k and of v
KT = 64                      # keys per tile of the forward / dq kernels
QR = 64                      # queries per stage of the dkv kernel
SCALE = 96 ** -0.5
LOG2E = math.log2(math.e)
LN2 = math.log(2.0)
KSC = SCALE * LOG2E          # what the pooling kernel multiplies the keys by
RESCALE_THR = 6.0            # the forward re-bases its running maximum only on jumps beyond 2^6 (attn_fwd.hip)
PEAK = 6.0                   # the peaked family: keys x 6 -> scores spread over 2-3 nat
READOUT_GAIN = 256.0         # exact in bf16; lifts P above the bf16 spacing of the residual
READOUT_BLOCK = 96           # keys read out per launch (one per value column)
BAR_FACTOR = 3.0             # a margin over the emulation's own error, not a measurement
LSE_BAR = 1e-3               # lse2, relative to max |lse2| (the bar the suite has always used)
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16


def rel_max(got, ref):
    got, ref = got.to(F64), ref.to(F64)
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-300))


def jeff(DA, J):
    return J if J > 0 else DA - HD


def fwd_ksu(DA, J):
    """k-steps of the forward's QK^T contraction (svit_attn_fwd: 6 + ceil(bias_cols / 16))."""
    return 6 + (jeff(DA, J) + 15) // 16


def bwd_ksu(DA, J):
    """the backward has two instantiations per DA (svit_attn_bwd: 7 | 8 at DA 128, 9 | 10 at DA 160)."""
    k = fwd_ksu(DA, J)
    return (7 if k <= 7 else 8) if DA == 128 else (9 if k <= 9 else 10)


def fwd_form(B, h, Nq, Nk, DA, J):
    """which forward kernel svit_attn_fwd launches: 'short' (Nk <= 64 and at most 8 k-steps), 'w8' (8 waves /
    3 stages: DA 160 and >= 200 workgroups of 256 queries), else 'w4' (4 waves / 2 stages)."""
    if Nk <= KT and fwd_ksu(DA, J) <= 8:
        return "short"
    wg8 = ((Nq + 255) // 256) * B * h
    return "w8" if DA == 160 and wg8 >= 200 else "w4"


def _residual(qa):
    r = qa[:, :HD].clone()
    r[0] = 0                 # the cls row takes no residual
    return r


# ------------------------------------------------------------------------------------------------ forward ----
def _target_tile(Nk):
    """the tile the tile-local mutants act on: the last FULL 64-key tile (tile 0 when there is none)."""
    return max(Nk // KT - 1, 0) * KT


def _target_step16(Nk):
    kb = _target_tile(Nk)
    lo = kb + (32 if Nk - kb > 32 else 0)
    return lo, min(lo + 16, Nk)


def _pad_keys(Nk):
    """rows a ragged last tile multiplies beyond Nk (a tile with <= 32 keys multiplies half a tile)."""
    rem = Nk % KT
    if rem == 0:
        return 0
    return (32 - rem) if rem <= 32 else (KT - rem)


def _tile_sweep(S, rescale_o):
    """the online softmax written out tile by tile with the forward's re-base rule (first tile always, later
    only on a jump of the running maximum beyond 2^RESCALE_THR).  rescale_o = False is the mutant that rescales
    the row sum but not the accumulator.  Returns the unnormalised weights as accumulated, l, m."""
    Nq, Nk = S.shape
    W = torch.zeros_like(S)
    l = torch.zeros(Nq, dtype=S.dtype)
    m = S[:, :KT].max(1).values
    for t0 in range(0, Nk, KT):
        St = S[:, t0:t0 + KT]
        if t0 > 0:
            jump = St.max(1).values - m
            shift = torch.where(jump > RESCALE_THR, jump, torch.zeros_like(jump))
            alpha = torch.exp2(-shift)
            l = l * alpha
            if rescale_o:
                W[:, :t0] *= alpha[:, None]
            m = m + shift
        Wt = torch.exp2(St - m[:, None])
        W[:, t0:t0 + KT] = Wt
        l = l + Wt.sum(1)
    return W, l, m


def _fwd_dense(qa, ka, J, mutant=None):
    """float64, one (batch, head): -> (M [Nq, Nk] with attention = M @ v, lse2 [Nq], residual [Nq, 96]).
    Every forward mutant is linear in v, so it is expressed through its M; the probability read-out of a
    mutant is then M itself."""
    qa, ka = qa.to(F64), ka.to(F64)
    Nq, DA = qa.shape
    Nk = ka.shape[0]
    S = qa @ ka.t()
    if mutant == "bias_kstep_ignored":           # ceil -> floor in the k-step count: the last step with data is lost
        lo = HD + 16 * ((jeff(DA, J) + 15) // 16 - 1)
        S = S - qa[:, lo:lo + 16] @ ka[:, lo:lo + 16].t()
    if mutant == "drop_ragged_tile":
        S = S[:, :(Nk - 1) // KT * KT]
    if mutant in ("no_rescale", "tile_sweep"):
        W, l, m = _tile_sweep(S, rescale_o=(mutant == "tile_sweep"))
    else:
        m = S.max(1).values
        W = torch.exp(S - m[:, None]) if mutant == "exp_not_exp2" else torch.exp2(S - m[:, None])
        l = W.sum(1)
    if mutant == "drop_ragged_tile":
        W = torch.cat([W, torch.zeros(Nq, Nk - W.shape[1], dtype=F64)], 1)
    if mutant == "v_rot_tile":                   # V rows of one tile rotated by one: key k meets the value of k + 1
        kb = _target_tile(Nk)
        n = min(KT, Nk - kb)
        W = W.clone()
        W[:, kb:kb + n] = torch.roll(W[:, kb:kb + n], 1, dims=1)
    if mutant in ("pv_skip16", "pv_skip32"):     # keys missing from P V, not from the row sum
        lo, hi = _target_step16(Nk)
        if mutant == "pv_skip32":
            hi = min(lo + 32, Nk)
        W = W.clone()
        W[:, lo:hi] = 0
    if mutant == "pad_keys_score0":              # the rows past Nk (re-reads of the last key) enter with score 0
        w0 = _pad_keys(Nk) * torch.exp2(-m)
        l = l + w0
        W = W.clone()
        W[:, Nk - 1] += w0
    res = qa[:, :HD].clone() if mutant == "residual_row0" else _residual(qa)
    return W / l[:, None], m + torch.log2(l), res


def fwd_mutant_applies(name, Nq, Nk, DA, J, family):
    if name == "drop_ragged_tile":
        return Nk % KT != 0 and Nk > KT
    if name == "no_rescale":                     # only planted keys make the maximum jump by 2^6 after the first tile
        return family == "peaked" and Nk > KT and bool(plants(Nq, Nk))
    if name == "pad_keys_score0":                # (in the peaked family 0 lies ~2^-11 below a row's maximum: no weight)
        return family == "flat" and _pad_keys(Nk) > 0
    if name == "v_rot_tile":
        return Nk >= 2
    if name == "residual_row0":                  # judged by the attention-only metric, which the peaked family carries
        return family == "peaked"
    return True


FWD_MUTANTS = ("v_rot_tile", "pv_skip16", "pv_skip32", "drop_ragged_tile", "pad_keys_score0", "no_rescale",
               "exp_not_exp2", "bias_kstep_ignored", "residual_row0")


def reference_fwd_2d(qa, ka, v, J=0, mutant=None):
    """-> (attn_only [Nq, 96], residual [Nq, 96], lse2 [Nq], P [Nq, Nk]), float64."""
    M, lse2, res = _fwd_dense(qa, ka, J, mutant)
    return M @ v.to(F64), res, lse2, M


def _bf(x):
    return x.to(BF16).to(F32)


def _emulate_p(qa, ka):
    """the rounding points up to the second product: fp32 scores of the bf16 operands, P = exp2(S - max)
    rounded to bf16, l summed over the rounded P."""
    q, k = qa.to(BF16).to(F32), ka.to(BF16).to(F32)
    S = q @ k.t()
    m = S.max(1).values
    Pb = _bf(torch.exp2(S - m[:, None]))
    l = Pb.sum(1)
    return Pb, l, m, _residual(q)


def emulate_fwd_2d(qa, ka, v):
    """-> (ctx bf16 [Nq, 96] residual included, as the kernel stores it; residual f32; lse2 f32)."""
    Pb, l, m, res = _emulate_p(qa, ka)
    attn = _bf((Pb @ v.to(BF16).to(F32)) * (1.0 / l)[:, None])      # staged in LDS as bf16 ...
    ctx = (attn + res).to(BF16)                                      # ... and rounded again behind the residual add
    ctx[0] = attn[0].to(BF16)
    return ctx, res, m + torch.log2(l)


def readout_of_ctx(ctx, res, block, Nk):
    """what a launch with v = READOUT_GAIN * one-hot(key - 96 * block) reveals: P[:, 96 block : 96 block + 96]."""
    n = min(READOUT_BLOCK, Nk - block * READOUT_BLOCK)
    return ((ctx.to(F64) - res.to(F64)) / READOUT_GAIN)[:, :n]


def readout_v(Nk, block, dtype=BF16):
    v = torch.zeros(Nk, HD, dtype=dtype)
    n = min(READOUT_BLOCK, Nk - block * READOUT_BLOCK)
    idx = torch.arange(n)
    v[block * READOUT_BLOCK + idx, idx] = READOUT_GAIN
    return v


def emulate_readout_2d(qa, ka):
    """the read-out of every key block at once: with a one-hot v the second product has ONE non-zero term per
    output, so ctx[:, c] = bf16(bf16(256 Pb[:, k] / l) + residual[:, c]) with c = k mod 96."""
    Pb, l, m, res = _emulate_p(qa, ka)
    Nk = ka.shape[0]
    attn = _bf((Pb * READOUT_GAIN) * (1.0 / l)[:, None])
    rk = res[:, torch.arange(Nk) % READOUT_BLOCK]
    ctx = _bf(attn + rk)
    return ((ctx.to(F64) - rk.to(F64)) / READOUT_GAIN), m + torch.log2(l)


# ----------------------------------------------------------------------------------------------- backward ----
BWD_MUTANTS = ("delta_missing", "delta_wrong_sign", "delta_with_residual", "dkv_lose_last8", "dq_skip32",
               "dk_no_scale", "dqa_bias_zero")


def bwd_mutant_applies(name, Nq, Nk, DA, J, family):
    if name == "dkv_lose_last8":                 # the last rows of a RAGGED 64-query stage
        return Nq % QR != 0 and Nq > 8
    if name == "delta_with_residual":
        return Nq > 1                            # row 0 carries no residual
    return True


def _split(dqa, dk, dv, DA, J):
    je = jeff(DA, J)
    return {"dq_main": dqa[:, :HD], "dq_bias": dqa[:, HD:HD + je], "dq_tail": dqa[:, HD + je:], "dk": dk, "dv": dv}


def reference_bwd_2d(qa, ka, v, dctx, J=0, scale=SCALE, mutant=None):
    """float64, written out: P = softmax, O = P v, delta = rowsum(dO O), dS = P (dP - delta);
    dqa = ln 2 dS ka, dk = scale dS^T q, dv = P^T dO.  -> dict dq_main | dq_bias | dq_tail | dk | dv."""
    qa, ka, v, dO = qa.to(F64), ka.to(F64), v.to(F64), dctx.to(F64)
    Nq, DA = qa.shape
    Nk = ka.shape[0]
    P, _, res = _fwd_dense(qa, ka, J)
    O = P @ v
    if mutant == "delta_with_residual":
        O = O + res
    delta = (dO * O).sum(1)
    if mutant == "delta_missing":
        delta = torch.zeros_like(delta)
    if mutant == "delta_wrong_sign":
        delta = -delta
    dS = P * (dO @ v.t() - delta[:, None])
    dS_q, dS_kv, P_kv = dS, dS, P
    if mutant == "dq_skip32":                    # the last 32-key step of the sweep
        lo = (Nk - 1) // 32 * 32
        dS_q = dS.clone()
        dS_q[:, lo:] = 0
    if mutant == "dkv_lose_last8":
        dS_kv, P_kv = dS.clone(), P.clone()
        dS_kv[Nq - 8:] = 0
        P_kv[Nq - 8:] = 0
    dqa = LN2 * (dS_q @ ka)
    if mutant == "dqa_bias_zero":
        dqa[:, HD:] = 0
    dk = (1.0 if mutant == "dk_no_scale" else scale) * (dS_kv.t() @ qa[:, :HD])
    dv = P_kv.t() @ dO
    return _split(dqa, dk, dv, DA, J)


def emulate_bwd_2d(qa, ka, v, ctx, dctx, lse2, J=0, scale=SCALE):
    """the backward kernels' rounding points: fp32 scores, P = exp2(S - lse2), delta from the bf16 ctx minus the
    residual, dS and P rounded to bf16 in front of the second products, fp32 accumulation; dqa leaves as bf16
    (x ln 2 applied to the finished fp32 tile), dk (x scale) and dv as fp32."""
    q, k, vv = qa.to(BF16).to(F32), ka.to(BF16).to(F32), v.to(BF16).to(F32)
    dO = dctx.to(BF16).to(F32)
    S = q @ k.t()
    P = torch.exp2(S - lse2.to(F32)[:, None])
    delta = (dO * (ctx.to(BF16).to(F32) - _residual(q))).sum(1)
    dSb = _bf(P * (dO @ vv.t() - delta[:, None]))
    dqa = _bf((dSb @ k) * LN2)
    dk = (dSb.t() @ q[:, :HD]) * scale
    dv = _bf(P).t() @ dO
    return _split(dqa, dk, dv, qa.shape[1], J)


BWD_TENSORS = ("dq_main", "dq_bias", "dk", "dv")


# ------------------------------------------------------------------------------------- [B, h, ...] wrappers ----
def slices(B, h):
    return [(b, hd) for b in range(B) for hd in range(h)]


def ctx_slice(ctx, b, hd):
    """ctx [B, Nq, h * 96] -> the [Nq, 96] of one (batch, head)."""
    return ctx[b, :, hd * HD:(hd + 1) * HD]


def reference_fwd(qa, ka, v, J=0):
    """[B,h,Nq,DA], [B,h,Nk,DA], [B,h,Nk,96] -> (attn_only [B,h,Nq,96], residual [B,h,Nq,96], lse2 [B,h,Nq],
    P [B,h,Nq,Nk]) in float64, one (batch, head) at a time."""
    B, h = qa.shape[:2]
    outs = [reference_fwd_2d(qa[b, hd], ka[b, hd], v[b, hd], J) for b, hd in slices(B, h)]
    return tuple(torch.stack([o[i] for o in outs]).reshape(B, h, *outs[0][i].shape) for i in range(4))


def reference_bwd(qa, ka, v, dctx, J=0, scale=SCALE):
    """dctx [B, Nq, h*96] -> dict of float64 [B,h,...] tensors (dq_main, dq_bias, dq_tail, dk, dv)."""
    B, h = qa.shape[:2]
    outs = [reference_bwd_2d(qa[b, hd], ka[b, hd], v[b, hd], ctx_slice(dctx, b, hd), J, scale) for b, hd in slices(B, h)]
    return {n: torch.stack([o[n] for o in outs]).reshape(B, h, *outs[0][n].shape) for n in outs[0]}


# --------------------------------------------------------------------------------------------------- cases ----
class Case:
    def __init__(self, name, B, h, Nq, Nk, DA, J):
        self.name, self.B, self.h, self.Nq, self.Nk, self.DA, self.J = name, B, h, Nq, Nk, DA, J
        self.form = fwd_form(B, h, Nq, Nk, DA, J)
        self.fwd_ksu, self.bwd_ksu = fwd_ksu(DA, J), bwd_ksu(DA, J)
        self.tiles = (Nk + KT - 1) // KT

    @property
    def shape(self):
        return (self.Nq, self.Nk, self.DA, self.J)

    def fwd_id(self):
        return "%s-fwd_%s_ksu%d-tiles%d" % (self.name, self.form, self.fwd_ksu, self.tiles)

    def __repr__(self):
        return "Case(%s B%d h%d Nq%d Nk%d DA%d J%d)" % (self.name, self.B, self.h, self.Nq, self.Nk, self.DA, self.J)


CASES = [
    # the step's own grids (16x224^2, B = 8) ...
    Case("step_blocks4_13", 8, 4, 1633, 457, 128, 22),               # 8 key tiles (ragged), automatic plan: 2 parts
    Case("step_block3", 8, 4, 1633, 1633, 160, 36),    # the 8-wave forward at its own grid, 26 tiles
    Case("step_blocks14_15", 8, 8, 457, 457, 128, 22),
    # ... and the frames pass
    Case("frames_J15", 2, 2, 300, 54, 128, 15),        # one ragged tile; ragged 128-row tile and wave block
    Case("frames_J29", 2, 2, 300, 201, 160, 29),       # 4 tiles; forward 8 k-steps at DA 160
    # tile counts and k-step counts
    Case("one_full_tile", 1, 1, 70, 64, 128, 32),
    Case("two_tiles_J15", 2, 2, 201, 128, 128, 15),
    Case("two_tiles_all_cols", 1, 1, 70, 128, 160, 64),
    Case("three_tiles_J0", 1, 1, 257, 192, 128, 0),                  # bias_cols unknown (0 = all); Nq = 2 * 128 + 1
    Case("six_tiles", 1, 2, 129, 330, 128, 22),
    Case("eight_tiles_all_cols", 2, 2, 300, 457, 160, 0),
    Case("tiles26_four_wave", 1, 2, 400, 1633, 160, 36),
    Case("half_tile_Nk20", 2, 2, 130, 20, 128, 9),     # at most 32 keys
    Case("Nk33_J30", 2, 3, 257, 33, 128, 30),
    Case("single_query_one_tile", 2, 3, 1, 64, 128, 15),
    Case("single_query_Nk457", 1, 2, 1, 457, 128, 22),
    # the 8-wave forward's other instantiations (>= 200 workgroups of 256 queries at DA 160)
    Case("wide_grid_J29", 25, 8, 130, 201, 160, 29),
    Case("wide_grid_all_cols", 25, 8, 200, 192, 160, 64),
]
CASE_BY_NAME = {c.name: c for c in CASES}


def plants(Nq, Nk):
    """(key, query row, gain): dominant keys of the peaked family.  One in the first tile, one in each of tiles
    1..3 (every slot of the two- and three-stage rings past the prologue), one in the last full tile, one at the
    very last key (the ragged tile), gains rising along the sweep so that the running maximum jumps by more than
    2^RESCALE_THR wherever a planted key arrives; row Nq - 2 is hit twice (two re-bases in one row) and lies, like
    Nq - 1, in the last 8 rows of the query range; row 0 is the cls row."""
    if Nq < 8:         # a handful of rows that are ALL one-hot would leave dS = P (dP - delta) = 0: nothing to measure
        return []
    nt = (Nk + KT - 1) // KT
    keys = [5] if Nk > 5 else []
    for t in sorted({1, 2, 3, Nk // KT - 1} | {0}):
        if 0 <= t < nt:
            keys.append(min(t * KT + 37, Nk - 1))
    keys.append(Nk - 1)
    keys = sorted(set(keys))
    rows = [Nq - 2, 3, Nq // 2, Nq - 2, 0, 7, Nq - 1]
    out = []
    for i, k in enumerate(keys):
        r = rows[i % len(rows)] if k != Nk - 1 else Nq - 1
        out.append((k, min(max(r, 0), Nq - 1), 4.0 + 2.0 * i))
    return out


def make_inputs(case, family, B=None):
    """deterministic bf16 inputs on the CPU: (qa, ka, v, dctx).  Element i of every tensor is a pure function of
    its name and i, so the tensors of a smaller B are the leading slices of those of a larger one."""
    B = case.B if B is None else B
    h, Nq, Nk, DA, J = case.h, case.Nq, case.Nk, case.DA, case.J
    tag = "%d_%d_%d" % (Nq, Nk, DA)
    qa = PR.tensor("ap:q" + tag, (B, h, Nq, DA), 1.0)
    ka = PR.tensor("ap:k" + tag, (B, h, Nk, DA), KSC)
    v = PR.tensor("ap:v" + tag, (B, h, Nk, HD), 1.0).to(BF16)
    dctx = PR.tensor("ap:d" + tag, (B, Nq, h * HD), 1.0).to(BF16)
    if family == "peaked":
        ka = ka * PEAK
    else:
        assert family == "flat"
    qa, ka = qa.to(BF16), ka.to(BF16)
    if family == "peaked":
        for k, r, gain in plants(Nq, Nk):
            ka[:, :, k] = (qa[:, :, r].float() * (gain * KSC)).to(BF16)
    if J:
        qa[..., HD + J:] = 0         # columns past J carry no data (the pooling kernel writes zeros)
        ka[..., HD + J:] = 0
    return qa, ka, v, dctx


REDUCED_HEADS = 2


def reduced_inputs(case, family):
    """the (batch 0, first two heads) slices the floor is measured on."""
    return tuple(t[:, :REDUCED_HEADS] if t.dim() == 4 else t[:, :, :REDUCED_HEADS * HD]
                 for t in make_inputs(case, family, B=1))


class Measure:
    """running max |got - ref| and max |ref| per named tensor over the slices of a case."""

    def __init__(self):
        self.err, self.ref = {}, {}

    def add(self, name, got, ref):
        got, ref = got.to(F64), ref.to(F64)
        self.err[name] = max(self.err.get(name, 0.0), float((got - ref).abs().max()))
        self.ref[name] = max(self.ref.get(name, 0.0), float(ref.abs().max()))

    def rel(self):
        return {n: self.err[n] / (self.ref[n] + 1e-300) for n in self.err}


def measure_case(case, family, fwd_variant, bwd_variant, qa, ka, v, dctx):
    """metrics of one implementation against the float64 reference over every (batch, head) of the given inputs.
    fwd_variant(qa2, ka2, v2) -> (ctx_or_attn, residual, lse2, readout [Nq, Nk] or None); the attention-only part is
    ctx - residual.  bwd_variant(qa2, ka2, v2, ctx2, dctx2, lse2) -> dict, or None.  Returns {tensor: rel}."""
    B, h = qa.shape[:2]
    ms = Measure()
    for b, hd in slices(B, h):
        q2, k2, v2 = qa[b, hd], ka[b, hd], v[b, hd]
        attn, res, lse2, P = reference_fwd_2d(q2, k2, v2, case.J)
        g_ctx, g_res, g_lse, g_read = fwd_variant(q2, k2, v2)
        if family == "peaked":
            ms.add("attn", g_ctx.to(F64) - g_res.to(F64), attn)
        ms.add("lse2", g_lse, lse2)
        if g_read is not None:
            ms.add("readout", g_read, P)
        if bwd_variant is not None:
            d2 = ctx_slice(dctx, b, hd)
            ref = reference_bwd_2d(q2, k2, v2, d2, case.J)
            got = bwd_variant(q2, k2, v2, g_ctx, d2, g_lse)
            for n in BWD_TENSORS:
                ms.add(n, got[n], ref[n])
    return ms.rel()


def emulated_fwd_variant(q2, k2, v2):
    ctx, res, lse2 = emulate_fwd_2d(q2, k2, v2)
    return ctx, res, lse2, emulate_readout_2d(q2, k2)[0]


def emulated_bwd_variant(case):
    return lambda q2, k2, v2, ctx, d2, lse2: emulate_bwd_2d(q2, k2, v2, ctx, d2, lse2, case.J)


def mutant_fwd_variant(case, name):
    def f(q2, k2, v2):
        attn, res, lse2, M = reference_fwd_2d(q2, k2, v2, case.J, mutant=name)
        true_res = _residual(q2.to(F64))             # what a test sees is ctx; it subtracts the TRUE residual
        cols = torch.arange(k2.shape[0]) % READOUT_BLOCK
        return attn + res, true_res, lse2, M + (res - true_res)[:, cols] / READOUT_GAIN
    return f


def mutant_bwd_variant(case, name):
    return lambda q2, k2, v2, ctx, d2, lse2: reference_bwd_2d(q2, k2, v2, d2, case.J, mutant=name)


def exact_fwd_variant(case):
    def f(q2, k2, v2):
        attn, res, lse2, M = reference_fwd_2d(q2, k2, v2, case.J)
        return attn + res, res, lse2, M
    return f


@functools.lru_cache(maxsize=None)
def case_floors(name, family):
    """metric(emulation, reference) per tensor on the reduced inputs of a case."""
    case = CASE_BY_NAME[name]
    qa, ka, v, dctx = reduced_inputs(case, family)
    return measure_case(case, family, emulated_fwd_variant, emulated_bwd_variant(case), qa, ka, v, dctx)


def case_bars(name, family):
    """the bar of every tensor of a case: BAR_FACTOR x the emulation's own distance from the reference; lse2 keeps
    the fixed bar the suite has always applied to it."""
    bars = {n: BAR_FACTOR * f for n, f in case_floors(name, family).items()}
    bars["lse2"] = LSE_BAR
    return bars


def attn_only_vs_bar(ctx, qa, ka, v, J=0):
    """for a test that already holds its own inputs: (max |(ctx - residual) - attention| / max |attention| over
    every (batch, head), its bar = BAR_FACTOR x the same figure of the emulation on the first two slices)."""
    ctx, qa, ka, v = (t.detach().cpu() for t in (ctx, qa, ka, v))
    B, h = qa.shape[:2]
    got, floor = Measure(), Measure()
    for i, (b, hd) in enumerate(slices(B, h)):
        attn, res, _, _ = reference_fwd_2d(qa[b, hd], ka[b, hd], v[b, hd], J)
        got.add("attn", ctx_slice(ctx, b, hd).to(F64) - res, attn)
        if i < REDUCED_HEADS:
            e_ctx, e_res, _ = emulate_fwd_2d(qa[b, hd], ka[b, hd], v[b, hd])
            floor.add("attn", e_ctx.to(F64) - e_res.to(F64), attn)
    return got.rel()["attn"], BAR_FACTOR * floor.rel()["attn"]
