"""Thin tensor-level wrappers over the C ABI (svit_amd/hip.py).

Every function enqueues HIP kernels on torch's current stream and returns torch tensors that
merely *own the memory*; no arithmetic here is done by PyTorch.
"""
import ctypes as C

import torch

from . import hip
from .hip import ptr

BF16 = torch.bfloat16
F32 = torch.float32
HD = 96
_scratch = {}


def scratch(device, floats=8 * 1024 * 1024, tag="main"):
    """Per-device fp32 scratch for the two-stage parameter-gradient reductions (32 MB); `tag`
    names an independent buffer for work that runs on another stream."""
    key = (device.index, floats, tag)
    buf = _scratch.get(key)
    if buf is None:
        buf = torch.empty(floats, device=device, dtype=F32)
        _scratch[key] = buf
    return buf


def _chk_rows(*ts):
    """2-D operands that may be column slices of a wider matrix (unit inner stride)."""
    for t in ts:
        if not t.is_cuda or t.dim() != 2 or t.stride(1) != 1:
            raise hip.SvitHipError("svit_amd GEMM operands must be 2-D device tensors with unit inner stride")


def _chk_dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise hip.SvitHipError("svit_amd ops need device tensors (got %s)" % t.device)
        if t is not None and not t.is_contiguous():
            raise hip.SvitHipError("svit_amd ops need contiguous tensors")


def gemm_nt(a, w, bias=None, epilogue=hip.EPI_BF16, out=None, out2=None, aux=None,
            row_scale=None, rows_per_sample=0, accumulate=False, remap=None, save=True, relq=None):
    """C = A[M,K] @ W[N,K]^T with a fused epilogue (see include/svit_hip.h).  `a` may be a
    column slice of a wider matrix (row-strided view).  epilogue EPI_RELQ: relq = (map i32 [Nq, extra],
    qa bf16 [..., Nq, 96 + extra], scale) -- the product is not stored, qa's rel-pos columns are written."""
    _chk_rows(a)
    _chk_dev(w, bias, out, out2, aux, row_scale)
    M, K = a.shape
    N = w.shape[0]
    assert w.shape[1] == K and a.dtype == BF16 and w.dtype == BF16
    if epilogue == hip.EPI_RELQ:
        cmap, qa, scale = relq
        _chk_dev(cmap, qa)
        extra = qa.shape[-1] - 96
        assert cmap.dtype == torch.int32 and cmap.is_contiguous() and cmap.shape == (qa.shape[-2], extra)
        assert qa.is_contiguous() and qa.numel() == M * qa.shape[-1] and bias is None
        g = hip.GemmArgs()
        g.A, g.lda, g.W, g.ldw = ptr(a), a.stride(0), ptr(w), w.stride(0)
        g.M, g.N, g.K, g.epilogue = M, N, K, epilogue
        g.relq_map, g.relq_out, g.relq_ld = ptr(cmap), ptr(qa), qa.shape[-1]
        g.relq_extra, g.relq_rows, g.relq_scale = extra, qa.shape[-2], scale
        hip.call("svit_gemm_nt", C.byref(g), meta=("mnk", M, N, K, epilogue, 2 * M * K + 2 * N * K + 2 * M * extra))
        return qa
    if out is None:
        dt = F32 if epilogue in (hip.EPI_RESID, hip.EPI_F32) else BF16
        out = torch.empty((M, N), device=a.device, dtype=dt)
    if epilogue == hip.EPI_GELU and out2 is None and save:
        out2 = torch.empty((M, N), device=a.device, dtype=BF16)
    g = hip.GemmArgs()
    g.A, g.lda, g.W, g.ldw = ptr(a), a.stride(0), ptr(w), w.stride(0)
    g.bias = ptr(bias)
    g.out, g.ldo = ptr(out), out.stride(-2)
    g.out2, g.ldo2 = ptr(out2), (out2.stride(-2) if out2 is not None else 0)
    g.aux, g.ldaux = ptr(aux), (aux.stride(-2) if aux is not None else 0)
    g.row_scale, g.rows_per_sample = ptr(row_scale), rows_per_sample
    g.M, g.N, g.K = M, N, K
    g.epilogue, g.accumulate = epilogue, int(accumulate)
    if remap is not None:
        g.remap_L, g.remap_N, g.remap_off = remap
    # algorithmic HBM bytes of the call (operands once, outputs once; residual / saved-derivative
    # slabs the epilogue reads): what bench.py prices against the 8 TB/s roof
    osz = out.element_size()
    nbytes = 2 * M * K + 2 * N * K + M * N * osz
    if out2 is not None:
        nbytes += 2 * M * N
    if aux is not None:
        nbytes += M * N * aux.element_size()
    if accumulate:
        nbytes += M * N * osz
    hip.call("svit_gemm_nt", C.byref(g), meta=("mnk", M, N, K, epilogue, nbytes))
    return (out, out2) if epilogue == hip.EPI_GELU else out


NT_FAMILIES = ("v2", "ring")
NT_RULES = ("forced", "ring_few_long_tiles", "ring_long_k_narrow", "bk64_narrow_long_k", "one_round_160x256",
            "one_round_192x192", "square_128x128", "big_128x192", "default_128x96")
_NT_PLAN_FIELDS = ("RB", "NB", "WM", "WN", "NL", "stages", "BK", "gx", "gy", "block", "lds")


def gemm_nt_plan(M, N, K, epilogue=hip.EPI_BF16):
    """Which kernel svit_gemm_nt would launch for this shape and epilogue under the current knobs, and how
    (svit_debug_gemm_nt_plan: the launch path's own chooser; launches nothing, needs no device) -> dict of family, the
    template parameters RB NB WM WN NL stages BK, grid gx gy, block, dynamic LDS bytes, and the rule that decided."""
    out = (C.c_int32 * 13)()
    n = hip.load().svit_debug_gemm_nt_plan(M, N, K, epilogue, out, 13)
    hip.check(min(n, 0), "svit_debug_gemm_nt_plan")
    plan = dict(zip(_NT_PLAN_FIELDS, out[1:12]))
    plan.update(family=NT_FAMILIES[out[0]], rule=NT_RULES[out[12]])
    return plan


def gemm_tn(a, b, dw, splits=0, dbias=None):
    """dw[N,K] (f32) += a[M,N]^T @ b[M,K].  a / b may be column slices (row-strided views)."""
    _chk_rows(a, b)
    _chk_dev(dw)
    M, N = a.shape
    K = dw.shape[-1]  # may be smaller than b's padded width (patch-embed wgrad)
    assert b.shape[0] == M and b.shape[1] >= K and dw.shape[-2] == N and dw.dtype == F32
    hip.call("svit_gemm_tn", ptr(a), a.stride(0), ptr(b), b.stride(0), ptr(dw), dw.stride(-2),
             M, N, K, splits, ptr(dbias), meta=("mnk", M, N, K))
    return dw


def _tn_problem_array(problems):
    """[(a[M,N], b[M,K'], dw[N,K] f32, dbias or None)], each as for gemm_tn -> (svit_tn_problem array, flop)"""
    arr = (hip.TnProblem * len(problems))()
    flop = 0.0
    for t, (a, b, dw, dbias) in zip(arr, problems):
        _chk_rows(a, b, dw)          # (dw too may be the leading columns of wider rows: lddw = its row stride)
        _chk_dev(dbias)
        M, N = a.shape
        K = dw.shape[1]  # may be smaller than b's padded width
        assert b.shape[0] == M and b.shape[1] >= K and dw.shape[0] == N and dw.dtype == F32
        t.A, t.B, t.dW, t.dbias = ptr(a), ptr(b), ptr(dw), ptr(dbias)
        t.lda, t.ldb, t.lddw, t.M, t.N, t.K = a.stride(0), b.stride(0), dw.stride(0), M, N, K
        flop += 2.0 * M * N * K
    return arr, flop


def gemm_tn_grouped(problems, ordered=False):
    """problems: [(a[M,N], b[M,K'], dw[N,K] f32, dbias or None)], each as for gemm_tn with a 2-D dw; all are accumulated
    by one launch per group of 16 (SVIT_TN_GROUP_MAX).  ordered: no split along the reduction rows (bit-reproducible
    weight gradients, slower)."""
    if not problems:
        return
    arr, flop = _tn_problem_array(problems)
    if ordered:
        hip.call("svit_gemm_tn_grouped_ex", arr, len(problems), 1, meta=("flop", flop))
    else:
        hip.call("svit_gemm_tn_grouped", arr, len(problems), meta=("flop", flop))


TN_FORMS = ("atomic", "ordered", "slab", "single")
_TN_PLAN_FIELDS = ("tile_kind", "tiles_n", "tiles_k", "rows_per_split", "splits", "first_block", "w", "tile_off", "bias_off",
                   "red_first")


def gemm_tn_plan(problems, form="atomic", splits=0):
    """What gemm_tn_grouped ("atomic"; "ordered"), gemm_tn_grouped_slab ("slab") or gemm_tn ("single": one problem, with
    `splits`) would launch for these problems under the current knobs (svit_debug_gemm_tn_plan: the launch path's own check
    and planners; launches nothing, needs no device).  problems: as for gemm_tn_grouped, or plain (M, N, K, has_bias) tuples
    (no tensors: fake aligned pointers and the smallest legal leading dimensions stand in).  form: a name or its index in
    TN_FORMS.  -> dict of form, workspace_floats (slab) and groups: per launch group grid, reduce_grid (slab) and problems,
    a dict each of tile_kind (0 = 128x96, 1 = 128x192), tiles_n, tiles_k, rows_per_split, splits, first_block and, for the
    slab form, w, tile_off, bias_off, red_first."""
    form = TN_FORMS.index(form) if isinstance(form, str) else form
    n = len(problems)
    if n and isinstance(problems[0][0], int):
        arr = (hip.TnProblem * n)()
        for t, (M, N, K, has_bias) in zip(arr, problems):
            t.A, t.B, t.dW, t.dbias = 1 << 20, 2 << 20, 3 << 20, (4 << 20) if has_bias else None
            t.lda, t.ldb, t.lddw, t.M, t.N, t.K = -(-N // 8) * 8, -(-K // 8) * 8, K, M, N, K
    else:
        arr = _tn_problem_array(problems)[0]
    size = 2 + 3 * (n // 16 + 1) + 10 * n
    out = (C.c_int64 * size)()
    got = hip.load().svit_debug_gemm_tn_plan(arr, n, form, splits, out, size)
    hip.check(min(got, 0), "svit_debug_gemm_tn_plan")
    vals, groups = iter(out[2:got]), []
    for _ in range(out[0]):
        count, grid, reduce_grid = next(vals), next(vals), next(vals)
        groups.append(dict(grid=grid, reduce_grid=reduce_grid,
                           problems=[dict(zip(_TN_PLAN_FIELDS, vals)) for _ in range(count)]))
    return dict(form=TN_FORMS[form], workspace_floats=out[1], groups=groups)


_tn_slab_need = {}      # shape set -> floats of slab workspace (the planner is a pure function of the shapes)
_tn_slab_ws = {}        # (device, tag) -> grow-only workspace


def gemm_tn_slab_workspace(arr, n, fresh=False):
    """floats of workspace svit_gemm_tn_grouped_slab needs for these problems (cached per shape set; fresh: ask again)"""
    key = tuple((t.M, t.N, t.K, t.dbias is not None) for t in arr)
    need = None if fresh else _tn_slab_need.get(key)
    if need is None:
        need = hip.load().svit_gemm_tn_grouped_workspace(arr, n)
        if need < 0:
            hip.check(need, "svit_gemm_tn_grouped_workspace")
        _tn_slab_need[key] = need
    return need


def _tn_slab_buffer(dev, tag, need):
    key = (dev.index, tag)
    ws = _tn_slab_ws.get(key)
    if ws is None or ws.numel() < need:
        if ws is not None:
            torch.cuda.synchronize(dev)      # launches still reading the buffer that is being replaced
        ws = _tn_slab_ws[key] = torch.empty(max(need, 1), device=dev, dtype=F32)
    return ws


def gemm_tn_grouped_slab(problems, ws=None, tag="tn_slab"):
    """gemm_tn_grouped without atomics: every row split stores its tile into a slab of `ws` and a second launch sums
    the slabs in split order -- for fixed shapes the result depends only on the operands (bit-reproducible run to run).
    ws=None: one grow-only buffer per (device, tag), sized on first use (so a captured step allocates nothing once its
    warm-up has run).  All slab calls that share a buffer must be on one stream: work on another stream names its own
    `tag`."""
    n = len(problems)
    if n == 0:
        return
    arr, flop = _tn_problem_array(problems)
    if ws is not None:
        _chk_dev(ws)
        assert ws.dtype == F32
        hip.call("svit_gemm_tn_grouped_slab", arr, n, ptr(ws), ws.numel(), meta=("flop", flop))
        return
    dev = problems[0][2].device
    ws = _tn_slab_buffer(dev, tag, gemm_tn_slab_workspace(arr, n))
    try:
        hip.call("svit_gemm_tn_grouped_slab", arr, n, ptr(ws), ws.numel(), meta=("flop", flop))
    except hip.SvitHipError:
        # refused before any launch.  A cached size goes stale when a tool turns the planner's knobs
        # (svit_debug_set_tn*): ask again, and only a size that really grew earns a second call
        need = gemm_tn_slab_workspace(arr, n, fresh=True)
        if need <= ws.numel():
            raise
        ws = _tn_slab_buffer(dev, tag, need)
        hip.call("svit_gemm_tn_grouped_slab", arr, n, ptr(ws), ws.numel(), meta=("flop", flop))


def gemm_tn_grouped_slab_lead(problems, shapes_behind, tag="tn_slab"):
    """gemm_tn_grouped_slab of `problems` planned as the head of a longer list (svit_gemm_tn_grouped_slab_lead):
    shapes_behind = [(M, N, K, has_bias)] of the problems that would follow them in the same call.  Only their shapes
    enter the plan; `problems` then get the row splits, and the bits, they have in the call over the whole list."""
    n, m = len(problems), len(shapes_behind)
    if m == 0:
        return gemm_tn_grouped_slab(problems, tag=tag)
    real, flop = _tn_problem_array(problems)
    arr = (hip.TnProblem * (n + m))()
    for i in range(n):
        arr[i] = real[i]
    for j, (M, N, K, has_bias) in enumerate(shapes_behind):      # (addresses that pass the checks and are never followed)
        t = arr[n + j]
        t.A, t.B, t.dW, t.dbias = 1 << 20, 2 << 20, 3 << 20, (4 << 20) if has_bias else None
        t.lda, t.ldb, t.lddw, t.M, t.N, t.K = -(-N // 8) * 8, -(-K // 8) * 8, K, M, N, K
    ws = _tn_slab_buffer(problems[0][2].device, tag, gemm_tn_slab_workspace(arr, n + m))
    hip.call("svit_gemm_tn_grouped_slab_lead", arr, n + m, n, ptr(ws), ws.numel(), meta=("flop", flop))


def reduce_defer(on):
    """queue (1) / run (0) the second-stage reduce launches of the backward kernels"""
    hip.call("svit_reduce_defer", int(on))


def reduce_flush():
    """run the current stream's queued second-stage reductions now (the stream stays in deferred mode)"""
    hip.call("svit_reduce_flush")


def reduce_reset():
    """error path: drop the current stream's queued reductions and leave deferred mode"""
    hip.call("svit_reduce_reset")


def colsum(a, out):
    _chk_dev(a, out)
    hip.call("svit_colsum_bf16", ptr(a), a.stride(0), ptr(out), a.shape[0], a.shape[1])
    return out


def cast_bf16(src, dst=None):
    _chk_dev(src, dst)
    if dst is None:
        dst = torch.empty(src.shape, device=src.device, dtype=BF16)
    hip.call("svit_cast_f32_bf16", ptr(src), ptr(dst), src.numel())
    return dst


def transpose_cast_batched(src_flat, dst_flat, table, n_mats, max_tiles):
    hip.call("svit_transpose_cast_batched", ptr(src_flat), ptr(dst_flat), ptr(table), n_mats,
             max_tiles)


def transpose_bf16_batched(src16_flat, dst_flat, table, n_mats, max_tiles):
    """the same table of [R,C] -> [C,R] transposes, read from the bf16 mirror (offsets index the mirror)"""
    _chk_dev(src16_flat, dst_flat, table)
    assert src16_flat.dtype == BF16 and dst_flat.dtype == BF16
    hip.call("svit_transpose_bf16_batched", ptr(src16_flat), ptr(dst_flat), ptr(table), n_mats,
             max_tiles)


def table_interp(mcat, tables, want_f32=True):
    """rel-pos tables at another resolution: (mcat f32 [Lp, J]) @ (tables f32 [J, 96]) -> (f32 [Lp, 96] or None, bf16 [Lp, 96])
    in one launch."""
    _chk_dev(mcat, tables)
    assert mcat.dtype == F32 and tables.dtype == F32 and mcat.is_contiguous() and tables.is_contiguous()
    assert mcat.shape[1] == tables.shape[0] and tables.shape[1] == HD
    r32 = torch.empty((mcat.shape[0], HD), device=mcat.device, dtype=F32) if want_f32 else None
    r16 = torch.empty((mcat.shape[0], HD), device=mcat.device, dtype=BF16)
    hip.call("svit_table_interp", ptr(mcat), mcat.shape[0], mcat.shape[1], ptr(tables), ptr(r32), ptr(r16))
    return r32, r16


def table_interp_jobs(entries, device):
    """entries: [(mcat f32 [Lp, J], tables f32 [J, 96], out32 f32 [Lp, 96] or None, out16 bf16 [Lp, 96])] -> the device
    descriptor table of svit_table_interp_batched (uint8 [n, 40]; keep it and every tensor it names alive)."""
    import struct
    raw = b"".join(struct.pack("<QQQQii", ptr(m), ptr(t), ptr(o32) or 0, ptr(o16) or 0, m.shape[0], m.shape[1])
                   for m, t, o32, o16 in entries)
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).view(len(entries), 40).to(device)


def table_interp_batched(jobs, max_rows):
    hip.call("svit_table_interp_batched", ptr(jobs), jobs.shape[0], max_rows)


def pad_cast_rows(src, dst):
    """dst bf16 [R,ldd] = [src f32 [R,C] | 0]."""
    _chk_dev(src, dst)
    hip.call("svit_pad_cast_rows", ptr(src), ptr(dst), src.shape[0], src.shape[1], dst.shape[1])
    return dst


def scale_cast(src, row_scale=None, rows_per_sample=0, dst=None, gather=None):
    """bf16(row_scale * src).  gather=(L, off): src is [B, N, C] and only rows [off, off+L) of
    every sample are converted -> dst [B*L, C]."""
    _chk_dev(src, row_scale, dst)
    cols = src.shape[-1]
    if gather is None:
        rows, gl, gn, go = src.shape[:-1].numel(), 0, 0, 0
        shape = src.shape
    else:
        gl, go = gather
        gn = src.shape[-2]
        rows = src.shape[0] * gl
        shape = (rows, cols)
    if dst is None:
        dst = torch.empty(shape, device=src.device, dtype=BF16)
    hip.call("svit_scale_cast", ptr(src), ptr(dst), ptr(row_scale), rows_per_sample, rows, cols,
             gl, gn, go)
    return dst


def layernorm_fwd(x, gamma, beta, eps=1e-6, want_f32=False, want_bf16=True, save_stats=True):
    _chk_dev(x, gamma, beta)
    C_ = x.shape[-1]
    rows = x.numel() // C_
    y16 = torch.empty(x.shape, device=x.device, dtype=BF16) if want_bf16 else None
    y32 = torch.empty(x.shape, device=x.device, dtype=F32) if want_f32 else None
    mean = torch.empty(rows, device=x.device, dtype=F32) if save_stats else None
    rstd = torch.empty(rows, device=x.device, dtype=F32) if save_stats else None
    hip.call("svit_layernorm_fwd", ptr(x), ptr(gamma), ptr(beta), ptr(y16), ptr(y32), ptr(mean),
             ptr(rstd), rows, C_, eps)
    return y16, y32, mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd, dgamma, dbeta, dres=None, dx=None, want_bf16=False,
                  row_scale=None, rows_per_sample=0, ws=None):
    """-> dx f32, or (dx, bf16(row_scale * dx)) with want_bf16 (operand of the next GEMM)."""
    _chk_dev(dy, x, gamma, mean, rstd, dgamma, dbeta, dres, dx, row_scale)
    C_ = x.shape[-1]
    rows = x.numel() // C_
    if dx is None:
        dx = torch.empty(x.shape, device=x.device, dtype=F32)
    dx16 = torch.empty(x.shape, device=x.device, dtype=BF16) if want_bf16 else None
    ws = scratch(x.device) if ws is None else ws
    assert dy.dtype in (F32, BF16)
    hip.call("svit_layernorm_bwd", ptr(dy), int(dy.dtype == BF16), ptr(x), ptr(gamma), ptr(mean),
             ptr(rstd), ptr(dres),
             ptr(dx), ptr(dx16), ptr(row_scale), rows_per_sample, ptr(dgamma), ptr(dbeta), rows, C_,
             ptr(ws), ws.numel())
    return (dx, dx16) if want_bf16 else dx


def im2col_patch(video):
    _chk_dev(video)
    B, Cin, T, H, W = video.shape
    assert Cin == 3 and video.dtype == F32
    To, Ho, Wo = (T - 1) // 2 + 1, (H - 1) // 4 + 1, (W - 1) // 4 + 1
    cols = torch.empty((B * To * Ho * Wo, 448), device=video.device, dtype=BF16)
    hip.call("svit_im2col_patch", ptr(video), ptr(cols), B, T, H, W)
    return cols, (To, Ho, Wo)


def patch_embed_dgrad(dtok16, w16, B, T, H, W, out=None):
    """The stem's data gradient (svit_patch_embed_dgrad): dtok16 bf16 [B*To*Ho*Wo, 96], the patch rows of block 0's dx,
    and w16 bf16 [96, 448], the forward's weight operand -> f32 [B,3,T,H,W], every element stored."""
    _chk_dev(dtok16, w16, out)
    To, Ho, Wo = (T - 1) // 2 + 1, (H - 1) // 4 + 1, (W - 1) // 4 + 1
    if dtok16.dtype != BF16 or tuple(dtok16.shape) != (B * To * Ho * Wo, HD):
        raise hip.SvitHipError("patch_embed_dgrad: dtok must be bf16 [%d, %d] for a clip [%d,3,%d,%d,%d], got %s %s"
                               % (B * To * Ho * Wo, HD, B, T, H, W, dtok16.dtype, tuple(dtok16.shape)))
    if w16.dtype != BF16 or tuple(w16.shape) != (HD, 448):
        raise hip.SvitHipError("patch_embed_dgrad: the weight operand must be bf16 [96, 448], got %s %s"
                               % (w16.dtype, tuple(w16.shape)))
    if out is None:
        out = torch.empty((B, 3, T, H, W), device=dtok16.device, dtype=F32)
    elif out.dtype != F32 or tuple(out.shape) != (B, 3, T, H, W):
        raise hip.SvitHipError("patch_embed_dgrad: out must be f32 %s, got %s %s"
                               % ((B, 3, T, H, W), out.dtype, tuple(out.shape)))
    hip.call("svit_patch_embed_dgrad", ptr(dtok16), ptr(w16), ptr(out), B, T, H, W)
    return out


def _chk_extents(extents, fr):
    """the per-video extents of an AugClips -> the `_ext` suffix and the extra argument; None: the plain entry point"""
    if extents is None:
        return "", ()
    if (extents.dtype != torch.int32 or tuple(extents.shape) != (fr.shape[0], 2) or not extents.is_contiguous()
            or extents.device != fr.device):
        raise hip.SvitHipError("the extents must be contiguous int32 [%d,2] on %s (got %s %s on %s)"
                               % (fr.shape[0], fr.device, extents.dtype, tuple(extents.shape), extents.device))
    return "_ext", (ptr(extents),)


def _im2col_u8(name, fr, lut, table, S, mix=(), frames_pass=False, extents=None):
    """One launch of a uint8 im2col kernel: frames u8 [V,T,Hs,Ws,3], its normalisation table, the per-clip table (crop
    rows or augmentation records) and, for the kernels that take one, the mix record (`mix` = (record or None,)).
    -> (cols bf16 [rows, 448], (To, Ho, Wo)); frames_pass: the B*T frames as single-frame clips; extents: the int32
    [V,2] table of the `_ext` form of an augmentation kernel."""
    _chk_dev(fr)
    V, T, Hs, Ws, _ = fr.shape
    B = table.shape[0]
    n, To = (B * T, 1) if frames_pass else (B, (T - 1) // 2 + 1)
    Ho = Wo = (S - 1) // 4 + 1
    cols = torch.empty((n * To * Ho * Wo, 448), device=fr.device, dtype=BF16)
    for m in mix:
        if m is not None:
            _chk_mix(m, fr.device)
    suffix, ext = _chk_extents(extents, fr)
    hip.call(name + suffix, ptr(fr), fr.numel(), ptr(lut), ptr(table), *ext, *[ptr(m) for m in mix], ptr(cols),
             B, T, Hs, Ws, S)
    return cols, (To, Ho, Wo)


def im2col_patch_u8(clips):
    """svit_amd.input.U8Clips -> the same [rows, 448] bf16 operand as im2col_patch."""
    mix = getattr(clips, "mix", None)
    if mix is not None:     # cfg.MIXUP on the uint8 route: blended / swapped between normalisation and bf16 rounding
        return _im2col_u8("svit_im2col_patch_u8_mix", clips.frames, clips.lut_f32, clips.crops, clips.size, (mix,))
    return _im2col_u8("svit_im2col_patch_u8", clips.frames, clips.lut, clips.crops, clips.size)


def _chk_aug(fr, rec, lut):
    """the frames, the int32 [B,16] record table and the fp32 table of an augment.AugClips on one device"""
    _chk_dev(fr, rec, lut)
    if rec.dtype != torch.int32 or rec.dim() != 2 or rec.shape[1] != 16 or not rec.is_contiguous() or rec.device != fr.device:
        raise hip.SvitHipError("the augmentation records must be contiguous int32 [B,16] on %s (got %s %s on %s)"
                               % (fr.device, rec.dtype, tuple(rec.shape), rec.device))
    if lut.dtype != F32 or lut.numel() != 768 or lut.device != fr.device:
        raise hip.SvitHipError("the normalisation table must be f32 [3,256] on %s" % (fr.device,))


def im2col_patch_u8_aug(clips):
    """svit_amd.augment.AugClips -> the same [rows, 448] bf16 operand as im2col_patch: resized crop, flip and erasing per
    the device records (and the mix of `clips.mix`, when set) between the fp32 normalisation and the one bf16 rounding."""
    _chk_aug(clips.frames, clips.records, clips.lut_f32)
    clips.run_randaug()         # (cfg.AUG.AA_TYPE: raw -> frames on this stream first; nothing without a table)
    return _im2col_u8("svit_im2col_patch_u8_aug", clips.frames, clips.lut_f32, clips.records, clips.size,
                      (getattr(clips, "mix", None),), extents=clips.extents)


def im2col_patch_u8_aug_frames(view):
    """svit_amd.input.FramesView -> the [B*T*Ho*Wo, 448] bf16 operand of im2col_patch for the B*T frames as single-frame
    clips [B*T,3,1,S,S] (svit_im2col_patch_u8_aug_frames): frame b*T + t through clip b's record, mixed per `view.mix`.
    An AugClips with a RandAugment table runs its chain first unless `view.fresh`; a U8Clips goes through the identity
    records of its crop table."""
    clips = view.clips
    if not view.fresh and hasattr(clips, "run_randaug"):
        clips.run_randaug()
    fr, rec, lut = view.frames, view.device_records(), view.lut_f32
    _chk_aug(fr, rec, lut)
    return _im2col_u8("svit_im2col_patch_u8_aug_frames", fr, lut, rec, view.size, (view.mix,), frames_pass=True,
                      extents=view.extents)


def u8_clips_render(clips):
    """svit_amd.augment.AugClips -> f32 [B,3,T,S,S]: the values im2col_patch_u8_aug rounds, unrounded (no mix)"""
    _chk_aug(clips.frames, clips.records, clips.lut_f32)
    clips.run_randaug()
    fr = clips.frames
    V, T, Hs, Ws, _ = fr.shape
    B, S = clips.records.shape[0], clips.size
    out = torch.empty((B, 3, T, S, S), device=fr.device, dtype=F32)
    suffix, ext = _chk_extents(clips.extents, fr)
    hip.call("svit_u8_clips_render" + suffix, ptr(fr), fr.numel(), ptr(clips.lut_f32), ptr(clips.records), *ext,
             ptr(out), B, T, Hs, Ws, S)
    return out


def feed_args(slot, frames, offsets=None, extents=None, fill=0, swap_rb=False, segments=(), slot_bytes=None):
    """The svit_feed_args of one launch (checked here for what the C side cannot see: devices, dtypes, shapes).
    slot: contiguous u8 device tensor (its first `slot_bytes` bytes are the slot; default: all of it); frames: u8
    [V,T,Hs,Ws,3]; offsets int64 [V] / extents int32 [V,2] on the device, or None; segments: up to eight
    (src_off, dst tensor[, bytes]) -- bytes defaults to the whole dst.  The struct holds raw pointers: keep the tensors."""
    _chk_dev(slot, frames, offsets, extents)
    if slot.dtype != torch.uint8 or frames.dtype != torch.uint8 or frames.dim() != 5 or frames.shape[-1] != 3:
        raise hip.SvitHipError("feed_unpack takes a uint8 slot and uint8 [V,T,Hs,Ws,3] frames, got %s and %s %s"
                               % (slot.dtype, frames.dtype, tuple(frames.shape)))
    V, T, Hs, Ws, _ = frames.shape
    if offsets is not None and (offsets.dtype != torch.int64 or tuple(offsets.shape) != (V,) or offsets.device != frames.device):
        raise hip.SvitHipError("the offsets must be int64 [%d] on %s" % (V, frames.device))
    if extents is not None:
        _chk_extents(extents, frames)
    a = hip.FeedArgs()
    a.slot, a.slot_bytes = ptr(slot), slot.numel() if slot_bytes is None else int(slot_bytes)
    if a.slot_bytes > slot.numel():
        raise hip.SvitHipError("slot_bytes %d exceeds the slot tensor's %d bytes" % (a.slot_bytes, slot.numel()))
    a.offsets, a.extents, a.frames = ptr(offsets), ptr(extents), ptr(frames)
    a.V, a.T, a.Hs, a.Ws, a.fill, a.swap_rb = V, T, Hs, Ws, int(fill), int(bool(swap_rb))
    if len(segments) > 8:
        raise hip.SvitHipError("feed_unpack carries at most 8 segments, got %d" % len(segments))
    a.n_seg = len(segments)
    for s, sg in enumerate(segments):
        dst = sg[1]
        _chk_dev(dst)
        if dst.device != frames.device:
            raise hip.SvitHipError("segment %d lives on %s, the frames on %s" % (s, dst.device, frames.device))
        full = dst.numel() * dst.element_size()
        nbytes = full if len(sg) < 3 else int(sg[2])
        if nbytes > full:
            raise hip.SvitHipError("segment %d: %d bytes into a tensor of %d" % (s, nbytes, full))
        a.seg[s].src_off, a.seg[s].dst, a.seg[s].bytes = int(sg[0]), ptr(dst), nbytes
    return a


def feed_unpack(args):
    """svit_feed_unpack on the current stream: one uploaded slot -> the padded frame buffer + the small segments
    (`feed_args`; svit_amd/feeder.py)."""
    hip.call("svit_feed_unpack", C.byref(args))


def _chk_mix(mix, device):
    """the 32-byte mix record (include/svit_hip.h, svit_mixup_clips): int32 [8] on the device of the data"""
    _chk_dev(mix)
    if mix.dtype != torch.int32 or mix.numel() != 8 or mix.device != device:
        raise hip.SvitHipError("the mix record must be int32 [8] on %s (got %s %s on %s)"
                               % (device, mix.dtype, tuple(mix.shape), mix.device))


def mixup_clips(x, mix):
    """x f32 contiguous [B, ..., H, W] mixed IN PLACE against the batch reversed, as the device record `mix` says
    (svit_mixup_clips: mixup blend, CutMix box swap, or nothing)."""
    _chk_dev(x)
    _chk_mix(mix, x.device)
    if x.dtype != F32 or x.dim() < 3:
        raise hip.SvitHipError("mixup_clips needs an fp32 [B, ..., H, W] tensor, got %s %s" % (x.dtype, tuple(x.shape)))
    B, H, W = x.shape[0], x.shape[-2], x.shape[-1]
    hip.call("svit_mixup_clips", ptr(x), ptr(mix), B, x[0].numel() // (H * W), H, W)
    return x


def _chk_attr_rec(rec, device):
    """the 32-byte pass record (include/svit_hip.h, svit_attr_pass): int32 [8] on the device of the data"""
    _chk_dev(rec)
    if rec.dtype != torch.int32 or rec.numel() != 8 or rec.device != device:
        raise hip.SvitHipError("the pass record must be int32 [8] on %s (got %s %s on %s)"
                               % (device, rec.dtype, tuple(rec.shape), rec.device))


def _chk_f32(what, t, shape, device):
    if t.dtype != F32 or tuple(t.shape) != tuple(shape) or t.device != device:
        raise hip.SvitHipError("%s must be f32 %s on %s, got %s %s on %s"
                               % (what, tuple(shape), device, t.dtype, tuple(t.shape), t.device))


def attr_perturb(x, rec, base=None, sigma=None, out=None):
    """svit_attr_perturb: out = base + alpha * (x - base) + sigma[b] * noise, every operation rounded once; x f32
    [B,3,T,H,W], base the same or None (zeros), sigma f32 [B] or None (no noise term), alpha and the seed of the noise
    field from the device record `rec`.  -> out (a fresh tensor unless given; it may not be x or base)."""
    _chk_dev(x, base, sigma, out)
    _chk_attr_rec(rec, x.device)
    if x.dtype != F32 or x.dim() != 5 or x.shape[1] != 3:
        raise hip.SvitHipError("attr_perturb takes an fp32 clip [B,3,T,H,W], got %s %s" % (x.dtype, tuple(x.shape)))
    B, _, T, H, W = x.shape
    if base is not None:
        _chk_f32("attr_perturb: base", base, x.shape, x.device)
    if sigma is not None:
        _chk_f32("attr_perturb: sigma", sigma, (B,), x.device)
    if out is None:
        out = torch.empty_like(x)
    else:
        _chk_f32("attr_perturb: out", out, x.shape, x.device)
        if out.data_ptr() == x.data_ptr() or (base is not None and out.data_ptr() == base.data_ptr()):
            raise hip.SvitHipError("attr_perturb: out may not be x or base")
    hip.call("svit_attr_perturb", ptr(x), ptr(base), ptr(sigma), ptr(rec), ptr(out), B, T, H, W)
    return out


def attr_accumulate(g, acc, rec, scores_in=None, scores=None):
    """svit_attr_accumulate: acc = (pass 0 ? 0 : acc) + weight * (g or g*g) as the device record `rec` says, g and acc
    f32 of one shape; with `scores` f32 [rows, B] the pass's scores `scores_in` f32 [B] are copied into row `pass`."""
    _chk_dev(g, acc, scores_in, scores)
    _chk_attr_rec(rec, g.device)
    if g.dtype != F32 or g.numel() < 1:
        raise hip.SvitHipError("attr_accumulate takes a non-empty fp32 gradient, got %s %s" % (g.dtype, tuple(g.shape)))
    _chk_f32("attr_accumulate: acc", acc, g.shape, g.device)
    rows, B = 0, g.shape[0]
    if scores is not None:
        if scores_in is None:
            raise hip.SvitHipError("attr_accumulate: a score table needs the pass's scores")
        B = scores_in.numel()
        _chk_f32("attr_accumulate: scores_in", scores_in, (B,), g.device)
        if scores.dim() != 2:
            raise hip.SvitHipError("attr_accumulate: the score table must be f32 [rows, %d]" % B)
        _chk_f32("attr_accumulate: scores", scores, (scores.shape[0], B), g.device)
        rows = scores.shape[0]
    hip.call("svit_attr_accumulate", ptr(g), ptr(acc), ptr(rec), ptr(scores_in if scores is not None else None),
             ptr(scores), rows, g.numel(), B)
    return acc


def fill_special_tokens(x, cls, objq, pos_t, L, Tx, O, add_pos):
    B, N, C_ = x.shape
    hip.call("svit_fill_special_tokens", ptr(x), ptr(cls), ptr(objq), ptr(pos_t), B, N, L, Tx, O,
             C_, int(add_pos))


def special_token_grads(dx, g_cls, g_obj, g_pos, L, Tx, O, add_pos):
    """gradients of cls_token / object_queries / pos_embed_temporal from d(block-0 input), ACCUMULATED, one launch"""
    B, N, C_ = dx.shape
    assert dx.is_contiguous() and dx.dtype == F32
    hip.call("svit_special_token_grads", ptr(dx), ptr(g_cls), ptr(g_obj), ptr(g_pos), B, N, L, Tx, O, C_, int(add_pos))


def pooled(n, s):
    return (n - 1) // s + 1


# no-grad passes over clips (T > 1: eval, multi-view test) hand the kernels a scratch pre / mean / rstd so that the pooling
# forward takes the same staged / slab launches as a training step (they hand `pre` from the conv launch to the LayerNorm
# launch); one-plane volumes (the frames pass) have their own kernel and keep nothing
NOGRAD_SCRATCH = True


def _pool_fwd_args(a, qkv, which, conv_w, gamma, beta, B, heads, thw, n_obj, stride_hw, ld_out, mode,
                   eps, save=True, out_scale=1.0):
    _chk_dev(qkv, conv_w, gamma, beta)
    T, H, W = thw
    Nout = 1 + T * pooled(H, stride_hw) * pooled(W, stride_hw) + n_obj
    dev = qkv.device
    out = torch.empty((B, heads, Nout, ld_out), device=dev, dtype=BF16)
    keep = save or (NOGRAD_SCRATCH and T > 1)
    pre = torch.empty((B, heads, Nout, HD), device=dev, dtype=BF16) if keep else None
    mean = torch.empty(B * heads * Nout, device=dev, dtype=F32) if keep else None
    rstd = torch.empty(B * heads * Nout, device=dev, dtype=F32) if keep else None
    a.qkv, a.which, a.conv_w, a.gamma, a.beta = ptr(qkv), which, ptr(conv_w), ptr(gamma), ptr(beta)
    a.out, a.ld_out, a.pre, a.mean, a.rstd = ptr(out), ld_out, ptr(pre), ptr(mean), ptr(rstd)
    a.B, a.heads, a.T, a.H, a.W, a.n_obj = B, heads, T, H, W, n_obj
    a.stride_hw, a.mode, a.eps, a.out_scale = stride_hw, mode, eps, out_scale
    return out, pre, mean, rstd       # (scratch included: the caller drops it AFTER the launch -- freed earlier, the next
                                      # tensor's `out` could be carved from the same block)


def pool_ln_fwd(qkv, which, conv_w, gamma, beta, B, heads, thw, n_obj, stride_hw, ld_out=HD,
                mode=0, eps=1e-6, out_scale=1.0):
    """-> out bf16 [B,h,Nout,ld_out], pre bf16 [B,h,Nout,96], mean, rstd f32 [B*h*Nout]."""
    a = hip.PoolArgs()
    res = _pool_fwd_args(a, qkv, which, conv_w, gamma, beta, B, heads, thw, n_obj, stride_hw,
                         ld_out, mode, eps, out_scale=out_scale)
    hip.call("svit_pool_ln_fwd", C.byref(a))
    return res


def pool_weight_sel(src_flat, offsets, dst):
    """selector tables (uint32 [n, 27, 96]) of n depthwise weights living at `offsets` (int64
    element offsets) of the fp32 buffer `src_flat` -- scalar operands of the tiled stencils."""
    _chk_dev(src_flat, offsets, dst)
    hip.call("svit_pool_weight_sel", ptr(src_flat), ptr(offsets), ptr(dst), offsets.numel())
    return dst


def _sel_ptrs(sels):
    arr = (C.c_void_p * 3)()
    for i in range(3):
        arr[i] = ptr(sels[i])
    return arr


def pool_ln_fwd_qkv(qkv, conv_ws, gammas, betas, B, heads, thw, n_obj, strides, ld_outs, modes,
                    eps=1e-6, save=True, sels=None, out_scales=(1.0, 1.0, 1.0), relq=None):
    """q, k, v pooling + LayerNorm in one launch -> [(out, pre, mean, rstd)] * 3 (the last three
    are None with save=False: no-grad passes keep nothing for a backward).  sels: the three
    selector tables (pool_weight_sel) -- stride-1 tensors then run the LDS-tiled stencil.
    relq = (rcat bf16 [Lpad, 96], map i32 [Nq, ld_out - 96], scale): the q tensor's rel-pos columns
    out[..., 96:] are written too (inside the slab LayerNorm kernel, or by a GEMM the entry point adds)."""
    arr = (hip.PoolArgs * 3)()
    res = [_pool_fwd_args(arr[i], qkv, i, conv_ws[i], gammas[i], betas[i], B, heads, thw, n_obj,
                          strides[i], ld_outs[i], modes[i], eps, save, out_scale=out_scales[i])
           for i in range(3)]
    if relq is not None:
        rcat, cmap, rscale = relq
        _chk_dev(rcat, cmap)
        assert rcat.dtype == BF16 and rcat.is_contiguous() and rcat.shape[1] == HD
        assert cmap.dtype == torch.int32 and cmap.is_contiguous()
        assert tuple(cmap.shape) == (res[0][0].shape[2], ld_outs[0] - HD)
        arr[0].relq_R, arr[0].relq_map, arr[0].relq_lpad, arr[0].relq_scale = ptr(rcat), ptr(cmap), rcat.shape[0], rscale
    if sels is None:
        hip.call("svit_pool_ln_fwd_qkv", arr)
    else:
        hip.call("svit_pool_ln_fwd_qkv_sel", arr, _sel_ptrs(sels))
    if not save:
        res = [(r[0], None, None, None) for r in res]
    return res


def _pool_ln_bwd_args(a, pre, mean, rstd, gamma, dgamma, dbeta, B, heads, Nout, d_main=None,
                      ld_main=HD, d_res=None, d_extra=None, ws=None):
    dpre = torch.empty((B, heads, Nout, HD), device=pre.device, dtype=BF16)
    a.d_main = ptr(d_main)
    a.main_is_f32 = int(d_main is not None and d_main.dtype == F32)
    a.ld_main = ld_main
    a.main_parts, a.main_part_stride = 1, 0
    if d_main is not None and d_main.dim() == 5:        # [parts, B, h, N, 96]: attn_bwd's partial planes
        assert d_main.dtype == F32
        a.main_parts, a.main_part_stride = d_main.shape[0], d_main.stride(0)
    a.d_res, a.d_extra = ptr(d_res), ptr(d_extra)
    a.extra_is_bf16 = int(d_extra is not None and d_extra.dtype == BF16)
    a.pre, a.mean, a.rstd, a.gamma = ptr(pre), ptr(mean), ptr(rstd), ptr(gamma)
    a.dpre, a.dgamma, a.dbeta = ptr(dpre), ptr(dgamma), ptr(dbeta)
    a.B, a.heads, a.Nout = B, heads, Nout
    ws = scratch(pre.device) if ws is None else ws
    a.workspace, a.workspace_floats = ptr(ws), ws.numel()
    return dpre


def pool_ln_bwd(pre, mean, rstd, gamma, dgamma, dbeta, B, heads, Nout, d_main=None, ld_main=HD,
                d_res=None, d_extra=None):
    a = hip.PoolLnBwdArgs()
    dpre = _pool_ln_bwd_args(a, pre, mean, rstd, gamma, dgamma, dbeta, B, heads, Nout, d_main,
                             ld_main, d_res, d_extra)
    hip.call("svit_pool_ln_bwd", C.byref(a))
    return dpre


def pool_ln_bwd_qkv(entries, ws=None):
    """entries: 3 x (args tuple, kwargs dict) of pool_ln_bwd -> [dpre] * 3, one launch."""
    arr = (hip.PoolLnBwdArgs * 3)()
    res = [_pool_ln_bwd_args(arr[i], *entries[i][0], ws=ws, **entries[i][1]) for i in range(3)]
    hip.call("svit_pool_ln_bwd_qkv", arr)
    return res


# (the four streaming conv-backward entry points left the product library in round 6: their wrappers live in
#  tools/diag/pool_streaming.py and need a -DSVIT_DIAG_POOL_STREAMING build)
def _pool_dgrad_args(a, dpre, conv_w, dqkv, which, B, heads, thw, n_obj, stride_hw):
    a.dpre, a.conv_w, a.dqkv, a.which = ptr(dpre), ptr(conv_w), ptr(dqkv), which
    a.B, a.heads, (a.T, a.H, a.W), a.n_obj, a.stride_hw = B, heads, thw, n_obj, stride_hw


def _pool_wgrad_args(a, dpre, qkv, which, dw, B, heads, thw, n_obj, stride_hw, ws=None):
    a.dpre, a.qkv, a.which, a.dw = ptr(dpre), ptr(qkv), which, ptr(dw)
    a.B, a.heads, (a.T, a.H, a.W), a.n_obj, a.stride_hw = B, heads, thw, n_obj, stride_hw
    ws = scratch(dpre.device) if ws is None else ws
    a.workspace, a.workspace_floats = ptr(ws), ws.numel()


def pool_conv_bwd_workspace(B, heads, thw, n_obj, strides):
    """floats of workspace pool_conv_bwd_qkv needs for this geometry (grows with the batch); -1 = no plan."""
    da = (hip.PoolDgradArgs * 3)()
    for i in range(3):
        da[i].B, da[i].heads, (da[i].T, da[i].H, da[i].W), da[i].n_obj, da[i].stride_hw, da[i].which = B, heads, thw, n_obj, strides[i], i
    return int(hip.load().svit_pool_conv_bwd_workspace(da))


POOL_PATHS = ("frame", "mfma", "slab", "staged", "stream")      # path codes of pool_plan(0, ...)
POOL_KERNELS = ("pool_frame_fwd", "pool_mfma_fwd", "pool_slab_fwd", "pool_slab_ln", "pool_fwd_staged", "pool_ln_fwd3")
POOL_RELQ = ("nobody", "pool_slab_ln", "gemm")


def pool_plan(kind, B, heads, thw, n_obj, strides, save=True, sels=False, relq_lpad=0):
    """What the host would decide for this geometry (svit_debug_pool_plan: launches nothing, needs no device).  kind 0: the
    forward of pool_ln_fwd_qkv -> (path, who writes q's rel-pos columns, [(kernel, grid x, y, z, block, LDS bytes)]);
    kind 1 / 2: the chunk plan of the staged forward / the fused backward -> {field: ints}, None where there is no plan."""
    out = (C.c_int32 * 24)()
    n = hip.load().svit_debug_pool_plan(kind, B, heads, *thw, n_obj, *strides, 7 if save else 0, int(sels), relq_lpad, out, 24)
    hip.check(min(n, 0), "svit_debug_pool_plan")
    if kind == 0:
        return POOL_PATHS[out[0]], POOL_RELQ[out[1]], [(POOL_KERNELS[out[i]],) + tuple(out[i + 1:i + 6]) for i in range(3, n, 6)]
    names = ("n_per", "r_per", "t_chunks", "y_chunks", "order")
    plan = {k: tuple(out[1 + 3 * i:4 + 3 * i]) for i, k in enumerate(names)}
    plan.update(first_item=tuple(out[16:20]), lds=out[20], max_chunks=out[21])
    return plan if out[0] else None


def pool_conv_bwd_qkv(dpres, conv_ws, dqkv, qkv, dws, B, heads, thw, n_obj, strides, ws=None):
    """conv dgrad + conv wgrad of q, k, v: one fused launch (csrc/pool.hip::pool_bwd_fused_kernel).  ws: the workspace of its
    partial rows (>= pool_conv_bwd_workspace(...) floats; it must outlive the deferred second-stage reduce); None = a per-device
    scratch of the needed size."""
    if ws is None:
        need = pool_conv_bwd_workspace(B, heads, thw, n_obj, strides)
        ws = scratch(dpres[0].device, max(8 * 1024 * 1024, need), tag="poolbwd")
    da = (hip.PoolDgradArgs * 3)()
    wa = (hip.PoolWgradArgs * 3)()
    for i in range(3):
        _pool_dgrad_args(da[i], dpres[i], conv_ws[i], dqkv, i, B, heads, thw, n_obj, strides[i])
        _pool_wgrad_args(wa[i], dpres[i], qkv, i, dws[i], B, heads, thw, n_obj, strides[i], ws)
    hip.call("svit_pool_conv_bwd_qkv", da, wa)


def relpos_q_fwd(qa, tabs, idx, B, heads, q_thw, k_thw, n_obj, inv_scale):
    a = hip.RelqArgs()
    a.qa, a.ld = ptr(qa), qa.shape[-1]
    a.rel_h, a.rel_w, a.rel_t = (ptr(t) for t in tabs)
    a.idx_h, a.idx_w, a.idx_t = (ptr(t) for t in idx)
    a.B, a.heads = B, heads
    a.qt, a.qh, a.qw = q_thw
    a.kt, a.kh, a.kw = k_thw
    a.n_obj, a.inv_scale = n_obj, inv_scale
    hip.call("svit_relpos_q_fwd", C.byref(a))


def relpos_q_bwd(qa, dqa, tabs, idx, dtabs, B, heads, q_thw, k_thw, n_obj, inv_scale):
    Nq = qa.shape[2]
    dq_extra = torch.empty((B, heads, Nq, HD), device=qa.device, dtype=F32)
    a = hip.RelqBwdArgs()
    a.qa, a.dqa, a.ld = ptr(qa), ptr(dqa), qa.shape[-1]
    a.rel_h, a.rel_w, a.rel_t = (ptr(t) for t in tabs)
    a.idx_h, a.idx_w, a.idx_t = (ptr(t) for t in idx)
    a.dq_extra = ptr(dq_extra)
    a.drel_h, a.drel_w, a.drel_t = (ptr(t) for t in dtabs)
    a.rows_h, a.rows_w, a.rows_t = (t.shape[0] for t in tabs)
    a.B, a.heads = B, heads
    a.qt, a.qh, a.qw = q_thw
    a.kt, a.kh, a.kw = k_thw
    a.n_obj, a.inv_scale = n_obj, inv_scale
    ws = scratch(qa.device)
    a.workspace, a.workspace_floats = ptr(ws), ws.numel()
    hip.call("svit_relpos_q_bwd", C.byref(a))
    return dq_extra


def relpos_gather(P, qa, idx, rows_off, B, heads, q_thw, k_thw, n_obj, inv_scale):
    """qa[..., 96 + j] = P[token, rows_off[sec] + idx] * inv_scale (see svit_relpos_gather)."""
    a = hip.RelqGatherArgs()
    a.P, a.ldp, a.qa, a.ld = ptr(P), P.shape[-1], ptr(qa), qa.shape[-1]
    a.idx_h, a.idx_w, a.idx_t = (ptr(t) for t in idx)
    a.row_h, a.row_w, a.row_t = rows_off
    a.B, a.heads = B, heads
    a.qt, a.qh, a.qw = q_thw
    a.kt, a.kh, a.kw = k_thw
    a.n_obj, a.inv_scale = n_obj, inv_scale
    hip.call("svit_relpos_gather", C.byref(a))


def relpos_scatter(dqa, idx, offs, ldd, B, heads, q_thw, k_thw, n_obj, inv_scale):
    """-> D bf16 [B*h*Nq, ldd] with d(relq)*inv_scale scattered to table-row columns."""
    Nq = dqa.shape[2]
    D = torch.empty((B * heads * Nq, ldd), device=dqa.device, dtype=BF16)
    a = hip.RelqScatterArgs()
    a.dqa, a.ld, a.D, a.ldd = ptr(dqa), dqa.shape[-1], ptr(D), ldd
    a.idx_h, a.idx_w, a.idx_t = (ptr(t) for t in idx)
    a.off_h, a.off_w, a.off_t = offs
    a.B, a.heads = B, heads
    a.qt, a.qh, a.qw = q_thw
    a.kt, a.kh, a.kw = k_thw
    a.n_obj, a.inv_scale = n_obj, inv_scale
    hip.call("svit_relpos_scatter", C.byref(a))
    return D


def attn_fwd(qa, ka, v, scale, bias_cols=0):
    """qa [B,h,Nq,DA], ka [B,h,Nk,DA], v [B,h,Nk,96] -> ctx bf16 [B,Nq,h*96], lse2 [B,h,Nq].
    bias_cols = kt + kh + kw (rel-pos columns that carry data; 0 = all DA - 96)."""
    _chk_dev(qa, ka, v)
    B, heads, Nq, DA = qa.shape
    Nk = ka.shape[2]
    ctx = torch.empty((B, Nq, heads * HD), device=qa.device, dtype=BF16)
    lse2 = torch.empty((B, heads, Nq), device=qa.device, dtype=F32)
    a = hip.AttnFwdArgs()
    a.qa, a.ka, a.v, a.ctx, a.lse2 = ptr(qa), ptr(ka), ptr(v), ptr(ctx), ptr(lse2)
    a.B, a.heads, a.Nq, a.Nk, a.DA, a.scale, a.bias_cols = B, heads, Nq, Nk, DA, scale, bias_cols
    hip.call("svit_attn_fwd", C.byref(a), meta=("attn", B, heads, Nq, Nk, DA))
    return ctx, lse2


def attn_bwd(qa, ka, v, ctx, dctx, lse2, scale, q_splits=0, bias_cols=0, reld=None):
    """-> dqa bf16 [B,h,Nq,DA], dk f32 [parts,B,h,Nk,96], dv f32 [parts,B,h,Nk,96]: the gradients of k
    and v are the SUMS over the leading axis (one plane per chunk of the query range; pool_ln_bwd
    adds them while it reads).  reld = (map i32 [Nq, DA - 96], ldd, scale[, rt]): the dq kernel also writes the
    rel-pos backward's scattered matrix D bf16 [B*h*Nq, ldd] (what relpos_scatter builds), returned 4th, and --
    given rt = the transposed tables bf16 [96, ldd], ldd <= 128 -- dq_extra = D . rt^T f32 [B*h*Nq, 96], returned
    5th (None when it was not computed: the caller then runs the GEMM); with a fifth element "fold" the product
    is added into dqa[..., :96] inside the kernel instead and the 5th result is the string "folded"."""
    _chk_dev(qa, ka, v, ctx, dctx, lse2)
    B, heads, Nq, DA = qa.shape
    Nk = ka.shape[2]
    dev = qa.device
    a = hip.AttnBwdArgs()
    a.B, a.heads, a.Nq, a.Nk, a.DA, a.q_splits, a.scale = B, heads, Nq, Nk, DA, q_splits, scale
    a.bias_cols = bias_cols
    parts = hip.load().svit_attn_bwd_parts(C.byref(a))
    if parts < 1:
        raise hip.SvitHipError("svit_attn_bwd_parts failed: %d" % parts)
    dqa = torch.empty((B, heads, Nq, DA), device=dev, dtype=BF16)
    dkv = torch.empty((2, parts, B, heads, Nk, HD), device=dev, dtype=F32)
    delta = torch.empty((B, heads, Nq, 2), device=dev, dtype=F32)
    a.qa, a.ka, a.v, a.ctx, a.dctx, a.lse2 = (ptr(t) for t in (qa, ka, v, ctx, dctx, lse2))
    a.delta, a.dqa, a.dk, a.dv = ptr(delta), ptr(dqa), ptr(dkv[0]), ptr(dkv[1])
    a.q_splits = parts
    D = X = None
    if reld is not None:
        cmap, ldd, rscale = reld[:3]
        rt = reld[3] if len(reld) > 3 else None      # bf16 [96, ldd]: also multiply dq_extra = D . rt^T
        _chk_dev(cmap, rt)
        assert cmap.dtype == torch.int32 and cmap.is_contiguous() and cmap.shape == (Nq, DA - HD)
        D = torch.empty((B * heads * Nq, ldd), device=dev, dtype=BF16)
        a.relD, a.relD_ld, a.relD_map, a.relD_scale = ptr(D), ldd, ptr(cmap), rscale
        mode = reld[4] if len(reld) > 4 else "separate"
        if rt is not None and ldd <= 128 and ldd % 16 == 0:
            assert rt.dtype == BF16 and rt.is_contiguous() and tuple(rt.shape) == (HD, ldd)
            a.relR = ptr(rt)
            if mode == "fold":        # dqa[:, :96] += D . rt^T inside the kernel: no dq_extra tensor at all
                X = "folded"
            else:
                X = torch.empty((B * heads * Nq, HD), device=dev, dtype=F32)
                a.relX = ptr(X)
    # (the D . R^T product of the rel-pos backward, when this launch carries it: 2 * rows * 96 * ldd flops that the
    # step used to spend in a GEMM launch of its own -- bench.py adds them to this kernel's algorithmic count)
    folded = 2.0 * B * heads * Nq * HD * reld[1] if (reld is not None and X is not None) else 0.0
    hip.call("svit_attn_bwd", C.byref(a), meta=("attn", B, heads, Nq, Nk, DA, folded))
    if reld is not None:
        return dqa, dkv[0], dkv[1], D, X
    return dqa, dkv[0], dkv[1]


def maxpool_fwd(x, thw, n_obj):
    B, N, C_ = x.shape
    T, H, W = thw
    Nout = 1 + T * pooled(H, 2) * pooled(W, 2) + n_obj
    y = torch.empty((B, Nout, C_), device=x.device, dtype=F32)
    idx = torch.empty((B, Nout, C_), device=x.device, dtype=torch.uint8)
    hip.call("svit_maxpool_fwd", ptr(x), ptr(y), ptr(idx), B, T, H, W, n_obj, C_)
    return y, idx


def maxpool_bwd(dy, idx, thw, n_obj, bf16=False):
    """bf16=True: dx rounded to bf16 (= scale_cast(maxpool_bwd(...)) bit for bit, one launch)."""
    B, Nout, C_ = dy.shape
    T, H, W = thw
    dx = torch.empty((B, 1 + T * H * W + n_obj, C_), device=dy.device, dtype=BF16 if bf16 else F32)
    hip.call("svit_maxpool_bwd_bf16" if bf16 else "svit_maxpool_bwd", ptr(dy), ptr(idx), ptr(dx),
             B, T, H, W, n_obj, C_)
    return dx


def sumsq(g, out):
    ws = scratch(g.device)
    hip.call("svit_sumsq", ptr(g), g.numel(), ptr(out), ptr(ws), ws.numel())


def adamw_step(p, g, m, v, sumsq_t, max_norm, lr, beta1, beta2, eps, wd, step, grad_scale=1.0):
    hip.call("svit_adamw_step", ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), ptr(sumsq_t), max_norm,
             lr, beta1, beta2, eps, wd, step, grad_scale)


def adamw_bias_table(beta1, beta2):
    """(bc1, bc2_sqrt) of AdamW steps 1, 2, ... as svit_adamw_step computes them on the host, up to the first step at
    which both are 1.0f: float32 numpy [entries, 2] (svit_adamw_bias_table; host only, needs no device)."""
    import numpy as np
    cap = 1 << 20
    buf = np.empty((cap, 2), dtype=np.float32)
    n = C.c_int64(0)
    rc = hip.load().svit_adamw_bias_table(beta1, beta2, buf.ctypes.data, cap, C.byref(n))
    hip.check(rc, "svit_adamw_bias_table (betas %r, %r)" % (beta1, beta2))
    return buf[:n.value].copy()


def _chk_step_records(host_rec, dev_rec, device):
    """the two parts of the step record (include/svit_hip.h: svit_step_host 32 bytes, svit_step_dev 48 bytes)"""
    _chk_dev(host_rec, dev_rec)
    if (host_rec.dtype != F32 or host_rec.numel() != 8 or dev_rec.dtype != torch.int32 or dev_rec.numel() != 12
            or host_rec.device != device or dev_rec.device != device):
        raise hip.SvitHipError("the step record is fp32 [8] + int32 [12] on %s" % (device,))


def step_guard(g, host_rec, dev_rec, table, workspace):
    """sum of squares of g + the decision of the step, written to dev_rec (svit_step_guard); table: fp32 [entries, 2]"""
    _chk_dev(g, table, workspace)
    _chk_step_records(host_rec, dev_rec, g.device)
    hip.call("svit_step_guard", ptr(g), g.numel(), ptr(host_rec), ptr(dev_rec), ptr(table), table.shape[0],
             ptr(workspace), workspace.numel())


def adamw_step_guarded(p, g, m, v, n_decay, host_rec, dev_rec, beta1, beta2, eps):
    """clip + AdamW of both weight-decay groups as the step record says, nothing on a dropped step"""
    _chk_dev(p, g, m, v)
    _chk_step_records(host_rec, dev_rec, p.device)
    n = p.numel()
    if g.numel() != n or m.numel() != n or v.numel() != n:
        raise hip.SvitHipError("adamw_step_guarded: p, g, m, v differ in size")
    hip.call("svit_adamw_step_guarded", ptr(p), ptr(g), ptr(m), ptr(v), n, n_decay, ptr(host_rec), ptr(dev_rec),
             beta1, beta2, eps)


def _chk_segs(segs):
    """the segment table of the `_seg` tail: a C-contiguous int64 numpy [S, 2] on the host (the library checks its contents)"""
    import numpy as np
    if not (isinstance(segs, np.ndarray) and segs.dtype == np.int64 and segs.ndim == 2 and segs.shape[1] == 2
            and segs.flags["C_CONTIGUOUS"]):
        raise hip.SvitHipError("the segment table is a C-contiguous int64 numpy array [S, 2]")
    return segs.ctypes.data, segs.shape[0]


def step_guard_seg(g, segs, host_rec, dev_rec, table, workspace):
    """step_guard over the segments of g only (svit_step_guard_seg): what lies outside is neither read nor counted"""
    _chk_dev(g, table, workspace)
    _chk_step_records(host_rec, dev_rec, g.device)
    sp, S = _chk_segs(segs)
    hip.call("svit_step_guard_seg", ptr(g), g.numel(), sp, S, ptr(host_rec), ptr(dev_rec), ptr(table), table.shape[0],
             ptr(workspace), workspace.numel())


def adamw_step_guarded_seg(p, g, m, v, n_decay, segs, host_rec, dev_rec, beta1, beta2, eps):
    """adamw_step_guarded on the elements inside the segments (svit_adamw_step_guarded_seg); nothing else is touched"""
    _chk_dev(p, g, m, v)
    _chk_step_records(host_rec, dev_rec, p.device)
    n = p.numel()
    if g.numel() != n or m.numel() != n or v.numel() != n:
        raise hip.SvitHipError("adamw_step_guarded_seg: p, g, m, v differ in size")
    sp, S = _chk_segs(segs)
    hip.call("svit_adamw_step_guarded_seg", ptr(p), ptr(g), ptr(m), ptr(v), n, n_decay, sp, S, ptr(host_rec),
             ptr(dev_rec), beta1, beta2, eps)


def adamw_step_guarded_lr(p, g, m, v, n_decay, segs, scales, host_rec, dev_rec, beta1, beta2, eps):
    """adamw_step_guarded_seg with the learning rate of segment s multiplied by scales[s], a C-contiguous float32 numpy
    [S] on the host (svit_adamw_step_guarded_lr; the library checks the contents of both tables before it launches)"""
    import numpy as np
    _chk_dev(p, g, m, v)
    _chk_step_records(host_rec, dev_rec, p.device)
    n = p.numel()
    if g.numel() != n or m.numel() != n or v.numel() != n:
        raise hip.SvitHipError("adamw_step_guarded_lr: p, g, m, v differ in size")
    sp, S = _chk_segs(segs)
    if not (isinstance(scales, np.ndarray) and scales.dtype == np.float32 and scales.shape == (S,)
            and scales.flags["C_CONTIGUOUS"]):
        raise hip.SvitHipError("the scales are a C-contiguous float32 numpy array [S], one per segment")
    hip.call("svit_adamw_step_guarded_lr", ptr(p), ptr(g), ptr(m), ptr(v), n, n_decay, sp, scales.ctypes.data, S,
             ptr(host_rec), ptr(dev_rec), beta1, beta2, eps)


def _chk_solver(what, segs, scales, host_rec, dev_rec, p, *others):
    """operands of the SGD / Adam tails: equal-sized device buffers (None where there is none), the step record, the range
    table and its scales -- None, or a C-contiguous float32 numpy [S] (the library checks the contents of both)"""
    import numpy as np
    _chk_dev(p, *others)
    _chk_step_records(host_rec, dev_rec, p.device)
    if any(t is not None and t.numel() != p.numel() for t in others):
        raise hip.SvitHipError("%s: the buffers differ in size" % what)
    sp, S = _chk_segs(segs)
    if scales is not None and not (isinstance(scales, np.ndarray) and scales.dtype == np.float32 and scales.shape == (S,)
                                   and scales.flags["C_CONTIGUOUS"]):
        raise hip.SvitHipError("the scales are None or a C-contiguous float32 numpy array [S], one per segment")
    return sp, None if scales is None else scales.ctypes.data, S


def sgd_step_guarded(p, g, buf, n_decay, segs, scales, host_rec, dev_rec, momentum, dampening, nesterov):
    """torch.optim.SGD's update on the ranges of `segs` as the step record says, nothing on a dropped step
    (svit_sgd_step_guarded); buf: the momentum buffer, None when momentum == 0; scales None: every scale 1.0"""
    sp, cp, S = _chk_solver("sgd_step_guarded", segs, scales, host_rec, dev_rec, p, g, buf)
    hip.call("svit_sgd_step_guarded", ptr(p), ptr(g), ptr(buf), p.numel(), n_decay, sp, cp, S, ptr(host_rec),
             ptr(dev_rec), momentum, dampening, int(bool(nesterov)))


def adam_step_guarded(p, g, m, v, n_decay, segs, scales, host_rec, dev_rec, beta1, beta2, eps):
    """torch.optim.Adam's update (coupled weight decay) on the ranges of `segs` (svit_adam_step_guarded)"""
    sp, cp, S = _chk_solver("adam_step_guarded", segs, scales, host_rec, dev_rec, p, g, m, v)
    hip.call("svit_adam_step_guarded", ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), n_decay, sp, cp, S, ptr(host_rec),
             ptr(dev_rec), beta1, beta2, eps)


def ema_decay_table(decay):
    """the warm-up decays of updates 1, 2, ...: min(decay, (1 + k) / (10 + k)) up to the first update that takes `decay`
    itself, float32 numpy [entries] (svit_ema_decay_table; host only, needs no device)"""
    import numpy as np
    lib = hip.load()
    n = C.c_int64(0)
    hip.check(lib.svit_ema_decay_table(decay, None, 0, C.byref(n)), "svit_ema_decay_table (decay %r)" % (decay,))
    buf = np.empty(n.value, dtype=np.float32)
    hip.check(lib.svit_ema_decay_table(decay, buf.ctypes.data, n.value, C.byref(n)),
              "svit_ema_decay_table (decay %r)" % (decay,))
    return buf


def ema_step_guarded(ema, p, segs, table, decay, ema_rec, dev_rec):
    """ema = ema * d + p * (1 - d) on the ranges of `segs` when the step record says the step was applied, nothing on a
    dropped step (svit_ema_step_guarded).  table: the warm-up decays as a float32 device tensor [entries], or None for
    the constant `decay`; ema_rec: int64 [2] on the device, {offset, reserved}; dev_rec: the guard's int32 [12]"""
    _chk_dev(ema, p, ema_rec, dev_rec)
    dev = p.device
    if ema.numel() != p.numel() or ema.dtype != F32 or p.dtype != F32 or ema.device != dev:
        raise hip.SvitHipError("ema_step_guarded: ema and p are fp32 buffers of one size on one device")
    if (ema_rec.dtype != torch.int64 or ema_rec.numel() != 2 or dev_rec.dtype != torch.int32 or dev_rec.numel() != 12
            or ema_rec.device != dev or dev_rec.device != dev):
        raise hip.SvitHipError("ema_step_guarded: the records are int64 [2] + int32 [12] on %s" % (dev,))
    entries = 0
    if table is not None:
        _chk_dev(table)
        if table.dtype != F32 or table.dim() != 1 or table.device != dev:
            raise hip.SvitHipError("ema_step_guarded: the decay table is a float32 tensor [entries] on %s" % (dev,))
        entries = table.numel()
    sp, S = _chk_segs(segs)
    hip.call("svit_ema_step_guarded", ptr(ema), ptr(p), p.numel(), sp, S, ptr(table) if entries else None, entries, decay,
             ptr(ema_rec), ptr(dev_rec))


def tensor_stats_window():
    """floats per window of svit_tensor_stats' first stage (host only)"""
    return int(hip.load().svit_tensor_stats_window())


def _chk_tensor_table(table):
    import numpy as np
    if not (isinstance(table, np.ndarray) and table.dtype == np.int64 and table.ndim == 2 and table.shape[1] == 2
            and table.flags["C_CONTIGUOUS"]):
        raise hip.SvitHipError("the tensor table is a C-contiguous int64 numpy array [Tn, 2]")
    return table.ctypes.data, table.shape[0]


def tensor_table_check(table, n):
    """svit_tensor_table_check: raises for a table the statistics kernels would refuse (host only, needs no device)"""
    tp, Tn = _chk_tensor_table(table)
    hip.check(hip.load().svit_tensor_table_check(tp, Tn, n), "svit_tensor_table_check (%d tensors, n = %d)" % (Tn, n))


def tensor_stats_workspace(n, Tn):
    """bytes of svit_tensor_stats' workspace for a buffer of n floats behind Tn tensors (host only)"""
    b = int(hip.load().svit_tensor_stats_workspace(n, Tn))
    if b < 0:
        hip.check(b, "svit_tensor_stats_workspace (n = %d, %d tensors)" % (n, Tn))
    return b


def _chk_step_dev(what, dev_rec, dev):
    if dev_rec.dtype != torch.int32 or dev_rec.numel() != 12 or dev_rec.device != dev:
        raise hip.SvitHipError("%s: the step record is int32 [12] on %s" % (what, dev))


def _chk_tensor_ring(what, names, bufs, table_dev, table_host, dev_rec, ring, R, entry_bytes, workspace):
    """what tensor_stats and update_stats check alike: `bufs` (None: absent) are fp32 buffers of one size on one device, the
    device table is the host's, the step record, a ring of R * (16 + entry_bytes * Tn) bytes and the workspace -> the host
    table's address, Tn"""
    _chk_dev(*bufs, table_dev, dev_rec, ring, workspace)
    n, dev = bufs[0].numel(), bufs[0].device
    tp, Tn = _chk_tensor_table(table_host)
    for t in bufs:
        if t is not None and (t.numel() != n or t.dtype != F32 or t.device != dev):
            raise hip.SvitHipError("%s: %s are fp32 buffers of one size on one device" % (what, names))
    if table_dev.dtype != torch.int64 or tuple(table_dev.shape) != (Tn, 2) or table_dev.device != dev:
        raise hip.SvitHipError("%s: the device table is int64 [%d, 2] on %s, as the host's" % (what, Tn, dev))
    _chk_step_dev(what, dev_rec, dev)
    if (ring.dtype != torch.uint8 or workspace.dtype != torch.uint8 or ring.device != dev or workspace.device != dev
            or R < 1 or ring.numel() != R * (16 + entry_bytes * Tn)):
        raise hip.SvitHipError("%s: the ring is uint8 [R * (16 + %d * %d)] and the workspace uint8, on %s"
                               % (what, entry_bytes, Tn, dev))
    return tp, Tn


def tensor_stats(g, p, table_dev, table_host, segs, dev_rec, ring, R, every, workspace):
    """per-tensor sums of squares of g and p, max |g|, count and first offset of the non-finite elements of g into row
    (step % R) of `ring`, when the step record says the step is due or was dropped (svit_tensor_stats; two launches).
    table_dev: int64 [Tn, 2] on the device, table_host: the same as numpy; segs: the trainable segments as numpy or None;
    ring: uint8 [R * (16 + 32 * Tn)] and workspace: uint8, both on the device"""
    tp, Tn = _chk_tensor_ring("tensor_stats", "g and p", (g, p), table_dev, table_host, dev_rec, ring, R, 32, workspace)
    sp, S = (None, 0) if segs is None else _chk_segs(segs)
    hip.call("svit_tensor_stats", ptr(g), ptr(p), g.numel(), ptr(table_dev), tp, Tn, sp, S, ptr(dev_rec), ptr(ring), R,
             every, ptr(workspace), workspace.numel())


def update_snapshot(p, shadow, segs, dev_rec, every):
    """shadow = p over the trainable segments (numpy or None: the whole buffer) when the step record says the step is due:
    applied, and its index a multiple of `every` (svit_update_snapshot; one launch)"""
    _chk_dev(p, shadow, dev_rec)
    dev = p.device
    if shadow.numel() != p.numel() or p.dtype != F32 or shadow.dtype != F32 or shadow.device != dev:
        raise hip.SvitHipError("update_snapshot: p and shadow are fp32 buffers of one size on one device")
    _chk_step_dev("update_snapshot", dev_rec, dev)
    sp, S = (None, 0) if segs is None else _chk_segs(segs)
    hip.call("svit_update_snapshot", ptr(p), ptr(shadow), p.numel(), sp, S, ptr(dev_rec), every)


def update_stats_workspace(n, Tn):
    """bytes of svit_update_stats' workspace for a buffer of n floats behind Tn tensors (host only)"""
    b = int(hip.load().svit_update_stats_workspace(n, Tn))
    if b < 0:
        hip.check(b, "svit_update_stats_workspace (n = %d, %d tensors)" % (n, Tn))
    return b


def update_stats(p, shadow, g, m, v, table_dev, table_host, segs, dev_rec, ring, R, every, workspace):
    """per-tensor statistics of the step p - shadow (and of p, g, m, v) into row (step % R) of `ring` when the step record
    says the step is due (svit_update_stats; two launches).  m, v: the moments or None; the tables as tensor_stats takes
    them; ring: uint8 [R * (16 + 64 * Tn)] and workspace: uint8, both on the device"""
    tp, Tn = _chk_tensor_ring("update_stats", "p, shadow, g, m and v", (p, shadow, g, m, v), table_dev, table_host, dev_rec,
                              ring, R, 64, workspace)
    sp, S = (None, 0) if segs is None else _chk_segs(segs)
    hip.call("svit_update_stats", ptr(p), ptr(shadow), ptr(g), ptr(m), ptr(v), p.numel(), ptr(table_dev), tp, Tn, sp, S,
             ptr(dev_rec), ptr(ring), R, every, ptr(workspace), workspace.numel())


def act_stats_window():
    """rows per window of svit_act_stats' first stage (host only)"""
    return int(hip.load().svit_act_stats_window())


def act_stats_workspace(total_windows):
    """bytes of svit_act_stats' workspace for a site table of that many windows (host only)"""
    b = int(hip.load().svit_act_stats_workspace(total_windows))
    if b < 0:
        hip.check(b, "svit_act_stats_workspace (%d windows)" % total_windows)
    return b


def act_site_table(sites, slots):
    """[(a, b or None, rows)] with a / b device addresses (ints) + the ring slot of each -> (svit_act_site array, int32
    slots as numpy): what the two calls below take.  Nothing is checked here."""
    import numpy as np
    tab = (hip.ActSite * max(1, len(sites)))()
    for i, (a, b, rows) in enumerate(sites):
        tab[i].a, tab[i].b, tab[i].rows, tab[i].first_window = a, b, rows, 0
    return tab, np.ascontiguousarray(np.asarray(slots, dtype=np.int32))


def act_sites_check(sites, slots, n_slots):
    """svit_act_sites_check: raises for a site table the statistics kernels would refuse (host only, needs no device)
    -> the table's windows"""
    import ctypes
    tab, sl = act_site_table(sites, slots)
    if len(sl) != len(sites):
        raise hip.SvitHipError("act_sites_check: one slot per site")
    windows = ctypes.c_int64(0)
    hip.check(hip.load().svit_act_sites_check(tab, sl.ctypes.data, len(sites), n_slots, ctypes.byref(windows)),
              "svit_act_sites_check (%d sites, %d slots)" % (len(sites), n_slots))
    return int(windows.value)


def act_stats(sites, slots, n_slots, geom, dev_rec, ring, R, state, workspace):
    """the forward statistics of one pass into row (pass % R) of `ring` (svit_act_stats; two launches).  sites:
    [(a, b or None, rows)] of device addresses, slots: their ring slots; geom: (B, Tx, T0, H0, W0); dev_rec: the guarded
    optimizer's int32 [12] record or None; ring: uint8 [R * (48 + 32 * n_slots)], state: int64 [1], workspace: uint8"""
    import numpy as np
    _chk_dev(ring, state, workspace)
    dev = ring.device
    if len(slots) != len(sites):
        raise hip.SvitHipError("act_stats: one slot per site")
    if dev_rec is not None:
        _chk_dev(dev_rec)
        _chk_step_dev("act_stats", dev_rec, dev)
    if state.dtype != torch.int64 or state.numel() != 1 or state.device != dev:
        raise hip.SvitHipError("act_stats: the pass counter is int64 [1] on %s" % (dev,))
    if (ring.dtype != torch.uint8 or workspace.dtype != torch.uint8 or workspace.device != dev or R < 1
            or n_slots < 1 or ring.numel() != R * (48 + 32 * n_slots)):
        raise hip.SvitHipError("act_stats: the ring is uint8 [R * (48 + 32 * %d)] and the workspace uint8, on %s"
                               % (n_slots, dev))
    g = np.ascontiguousarray(np.asarray(geom, dtype=np.int32))
    if g.shape != (5,):
        raise hip.SvitHipError("act_stats: geom is (B, Tx, T0, H0, W0)")
    tab, sl = act_site_table(sites, slots)
    hip.call("svit_act_stats", tab, sl.ctypes.data, len(sites), n_slots, g.ctypes.data, ptr(dev_rec), ptr(ring), R,
             ptr(state), ptr(workspace), workspace.numel())


ATTN_GROUP_KINDS = {"cls": 0, "obj": 1, "patch": 2}


def attn_stats_workspace(total_wgs):
    """bytes of svit_attn_stats' workspace for a site table of that many stage-1 workgroups (host only)"""
    b = int(hip.load().svit_attn_stats_workspace(total_wgs))
    if b < 0:
        hip.check(b, "svit_attn_stats_workspace (%d workgroups)" % total_wgs)
    return b


def attn_site_table(sites, groups, K, every, maps_samples):
    """sites: [dict(qa, ka, lse2, maps (device addresses, maps may be None), B, heads, Nq, Nk, DA, bias_cols, Lq, Lk,
    n_obj, slot, ent_base)]; groups: kinds in entry order (0 cls, 1 obj, 2 patch) -> (svit_attn_site array,
    svit_attn_probe): what the two calls below take.  Nothing is checked here beyond the number of groups."""
    tab = (hip.AttnSite * max(1, len(sites)))()
    for i, s in enumerate(sites):
        t = tab[i]
        t.qa, t.ka, t.lse2, t.maps = s["qa"], s["ka"], s["lse2"], s.get("maps")
        for k in ("B", "heads", "Nq", "Nk", "DA", "bias_cols", "Lq", "Lk", "n_obj", "slot", "ent_base"):
            setattr(t, k, s[k])
        t.first_wg = 0
    probe = hip.AttnProbe()
    if len(groups) > 3:
        raise hip.SvitHipError("attn_site_table: at most 3 query groups, got %d" % len(groups))
    probe.n_groups = len(groups)
    for i, k in enumerate(groups):
        probe.kind[i] = k
    probe.K, probe.every, probe.maps_samples, probe.reserved = K, every, maps_samples, 0
    return tab, probe


def attn_sites_check(sites, n_slots, ent_slots, groups, K=32, every=1, maps_samples=0):
    """svit_attn_sites_check: raises for a site table or a probe the attention statistics would refuse (host only, needs
    no device) -> the workgroups of stage 1"""
    import ctypes
    tab, probe = attn_site_table(sites, groups, K, every, maps_samples)
    wgs = ctypes.c_int64(0)
    hip.check(hip.load().svit_attn_sites_check(tab, len(sites), n_slots, ent_slots, ctypes.byref(probe),
                                               ctypes.byref(wgs)),
              "svit_attn_sites_check (%d sites, %d slots, %d entries)" % (len(sites), n_slots, ent_slots))
    return int(wgs.value)


def attn_stats(sites, n_slots, ent_slots, groups, K, every, maps_samples, geom, dev_rec, ring, R, state, workspace):
    """the attention statistics of one pass into row (rows written % R) of `ring` when the pass is due (svit_attn_stats;
    two launches).  sites, groups: as attn_site_table takes them; geom: (B, Tx, T0, H0, W0); dev_rec: the guarded
    optimizer's int32 [12] record or None; ring: uint8 [R * (48 + 64 * ent_slots)], state: int64 [4], workspace: uint8"""
    import ctypes
    import numpy as np
    _chk_dev(ring, state, workspace)
    dev = ring.device
    if dev_rec is not None:
        _chk_dev(dev_rec)
        _chk_step_dev("attn_stats", dev_rec, dev)
    if state.dtype != torch.int64 or state.numel() != 4 or state.device != dev:
        raise hip.SvitHipError("attn_stats: the counters are int64 [4] on %s" % (dev,))
    if (ring.dtype != torch.uint8 or workspace.dtype != torch.uint8 or workspace.device != dev or R < 1
            or ent_slots < 1 or ring.numel() != R * (48 + 64 * ent_slots)):
        raise hip.SvitHipError("attn_stats: the ring is uint8 [R * (48 + 64 * %d)] and the workspace uint8, on %s"
                               % (ent_slots, dev))
    g = np.ascontiguousarray(np.asarray(geom, dtype=np.int32))
    if g.shape != (5,):
        raise hip.SvitHipError("attn_stats: geom is (B, Tx, T0, H0, W0)")
    tab, probe = attn_site_table(sites, groups, K, every, maps_samples)
    hip.call("svit_attn_stats", tab, len(sites), n_slots, ent_slots, ctypes.byref(probe), g.ctypes.data, ptr(dev_rec),
             ptr(ring), R, ptr(state), ptr(workspace), workspace.numel())


# ---------------------------------------------------------------- head (K15) ----------------
def _head_args(tokens, T, O, keep, head_params, outs):
    a = hip.HeadArgs()
    B, N, C_ = tokens.shape
    a.tokens, a.B, a.N, a.C, a.T, a.O = ptr(tokens), B, N, C_, T, O
    a.keep = ptr(keep)
    (wp, bp), (wb, bb), (we, be), (wc, bc) = head_params
    a.w_proj, a.b_proj, a.n_cls = ptr(wp), ptr(bp), wp.shape[0]
    a.w_box, a.b_box, a.w_bce, a.b_bce, a.w_con, a.b_con = ptr(wb), ptr(bb), ptr(we), ptr(be), ptr(wc), ptr(bc)
    a.logits, a.boxes, a.contact, a.xobj = (ptr(t) for t in outs)
    return a


def head_fwd(tokens, T, O, keep, head_params):
    """SViT head in one launch (svit_head_fwd): tokens f32 [B,N,C] -> logits [B,n_cls], pred_bboxes [B,T,O,5],
    contact [B,T,2,5], obj_desc [B,T,O,C].  head_params = ((w,b) of projection, box MLP, objectness, contact)."""
    assert tokens.is_contiguous() and tokens.dtype == F32
    _chk_dev(tokens, keep, *[t for wb in head_params for t in wb])
    B, N, C_ = tokens.shape
    dev = tokens.device
    outs = (torch.empty((B, head_params[0][0].shape[0]), device=dev), torch.empty((B, T, O, 5), device=dev),
            torch.empty((B, T, 2, 5), device=dev), torch.empty((B, T, O, C_), device=dev))
    a = _head_args(tokens, T, O, keep, head_params, outs)
    hip.call("svit_head_fwd", C.byref(a))
    return outs


def head_eval(tokens, T, O, head_params, act=0):
    """The eval-mode head in one launch (svit_head_eval): tokens f32 [B,N,C] as Engine.forward returns them -> class
    PROBABILITIES [B,n_cls] (act 0 softmax, 1 sigmoid), pred_bboxes [B,T,O,5] (column 0 the sigmoid of the objectness
    logit), contact [B,T,2,5] softmaxed over its last axis, obj_desc [B,T,O,C]."""
    if not tokens.is_contiguous() or tokens.dtype != F32 or tokens.dim() != 3:
        raise hip.SvitHipError("head_eval takes contiguous f32 [B,N,C] tokens, got %s %s" % (tokens.dtype, tuple(tokens.shape)))
    _chk_dev(tokens, *[t for wb in head_params for t in wb])
    B, N, C_ = tokens.shape
    dev = tokens.device
    outs = (torch.empty((B, head_params[0][0].shape[0]), device=dev), torch.empty((B, T, O, 5), device=dev),
            torch.empty((B, T, 2, 5), device=dev), torch.empty((B, T, O, C_), device=dev))
    a = _head_args(tokens, T, O, None, head_params, outs)
    hip.call("svit_head_eval", C.byref(a), int(act))
    return outs


def head_bwd(tokens, T, O, keep, head_params, boxes, grads_out, param_grads, ordered=False):
    """-> d(tokens) f32 [B,N,C] (zero rows for the patch tokens); the parameter gradients are ADDED into
    param_grads (same nesting as head_params).  grads_out = (dlogits, dboxes, dcontact, dxobj), None allowed.
    ordered: the box / contact gradients are summed over the object rows in a fixed order (no atomics)."""
    assert tokens.is_contiguous() and tokens.dtype == F32
    go = [None if t is None else t.contiguous() for t in grads_out]
    _chk_dev(tokens, keep, boxes, *[t for t in go if t is not None])
    g = hip.HeadBwdArgs()
    # of the forward outputs only the sigmoid boxes are read; the argument check wants the three pointers set
    g.f = _head_args(tokens, T, O, keep, head_params, (boxes, boxes, boxes, None))
    g.dlogits, g.dboxes, g.dcontact, g.dxobj = (ptr(t) for t in go)
    dtok = torch.empty_like(tokens)
    g.dtokens = ptr(dtok)
    (gwp, gbp), (gwb, gbb), (gwe, gbe), (gwc, gbc) = param_grads
    g.gw_proj, g.gb_proj, g.gw_box, g.gb_box = ptr(gwp), ptr(gbp), ptr(gwb), ptr(gbb)
    g.gw_bce, g.gb_bce, g.gw_con, g.gb_con = ptr(gwe), ptr(gbe), ptr(gwc), ptr(gbc)
    g.ordered = int(ordered)
    hip.call("svit_head_bwd", C.byref(g))
    return dtok


# ---------------------------------------------------------------- image-rank HAOG losses ----
def haog_loss_fwd(pred, tar, contact, contact_tar):
    """-> (losses f32 [8], (g_l1, g_bce, g_giou, g_contact)); see include/svit_hip.h."""
    R, Rc = pred.numel() // 5, contact.numel() // 5
    assert pred.dtype == F32 and tar.dtype == F32 and contact.dtype == F32
    assert contact_tar.dtype == torch.int64 and tar.numel() == R * 4 and contact_tar.numel() == Rc
    dev = pred.device
    losses = torch.empty(8, dtype=F32, device=dev)
    g_l1, g_giou = torch.empty((R, 4), dtype=F32, device=dev), torch.empty((R, 4), dtype=F32, device=dev)
    g_bce, g_contact = torch.empty(R, dtype=F32, device=dev), torch.empty((Rc, 5), dtype=F32, device=dev)
    hip.call("svit_haog_loss", ptr(pred), ptr(tar), ptr(contact), ptr(contact_tar), ptr(losses),
             ptr(g_l1), ptr(g_bce), ptr(g_giou), ptr(g_contact), R, Rc)
    return losses, (g_l1, g_bce, g_giou, g_contact)


def haog_loss_bwd(upstream, unit, pred_shape, contact_shape):
    g_l1, g_bce, g_giou, g_contact = unit
    R, Rc = g_bce.numel(), g_contact.numel() // 5
    dpred = torch.empty(pred_shape, dtype=F32, device=g_bce.device)
    dcontact = torch.empty(contact_shape, dtype=F32, device=g_bce.device)
    hip.call("svit_haog_loss_bwd", ptr(upstream), ptr(g_l1), ptr(g_bce), ptr(g_giou),
             ptr(g_contact), ptr(dpred), ptr(dcontact), R, Rc)
    return dpred, dcontact


def ce_loss(logits, labels):
    """mean cross entropy over the rows (ignore_index -100) and d loss / d logits in one launch (svit_ce_loss)."""
    _chk_dev(logits, labels)
    assert logits.dtype == F32 and logits.dim() == 2 and labels.dtype == torch.int64 and labels.numel() == logits.shape[0]
    logits, labels = logits.contiguous(), labels.contiguous()
    loss = torch.empty((), device=logits.device, dtype=F32)
    dlogits = torch.empty_like(logits)
    hip.call("svit_ce_loss", ptr(logits), ptr(labels), logits.shape[0], logits.shape[1], ptr(loss), ptr(dlogits))
    return loss, dlogits


def ce_loss_soft(logits, target=None, labels=None, mix=None, on=1.0, off=0.0):
    """cross entropy against a soft target and d loss / d logits in one launch (svit_ce_loss_soft).  Either `target` f32 [B,C]
    (dense) or `labels` int64 [B] (+ the device mix record, + the smoothed one-hot values on / off): the target of
    mixup.MixUp is then built in registers, t = v(labels) * lam + v(labels reversed) * (1 - lam)."""
    _chk_dev(logits, target, labels)
    assert logits.dtype == F32 and logits.dim() == 2
    B, C_ = logits.shape
    if (target is None) == (labels is None):
        raise hip.SvitHipError("ce_loss_soft takes a dense target or labels, not both / neither")
    if target is not None:
        assert target.dtype == F32 and target.shape == logits.shape and mix is None
    else:
        assert labels.dtype == torch.int64 and labels.numel() == B
        if mix is not None:
            _chk_mix(mix, logits.device)
    loss = torch.empty((), device=logits.device, dtype=F32)
    dlogits = torch.empty_like(logits)
    hip.call("svit_ce_loss_soft", ptr(logits), ptr(target), ptr(labels), ptr(mix), float(on), float(off), B, C_,
             ptr(loss), ptr(dlogits))
    return loss, dlogits


def step_draws(state, keep, per_block, n_drop=0, p_drop=0.0):
    """state int64 [3] = {seed, draw number, 0} (advanced by the launch); keep f32 [n_blocks] -> scales f32 [n_blocks, per_block] =
    floor(keep + U) / keep and drop f32 [n_drop] in {0, 1 / (1 - p)} (svit_step_draws; one launch)."""
    _chk_dev(state, keep)
    assert state.dtype == torch.int64 and state.numel() == 3 and keep.dtype == F32
    nb = keep.numel()
    scales = torch.empty((nb, per_block), device=state.device, dtype=F32)
    drop = torch.empty((n_drop,), device=state.device, dtype=F32) if n_drop else None
    hip.call("svit_step_draws", ptr(state), ptr(keep), nb, per_block, ptr(scales), n_drop, float(p_drop), ptr(drop))
    return scales, drop
