"""svit_gemm_nt against the float64 reference of tests/gemm_reference.py, element by element, on every epilogue path
of every kernel form, with bars derived from the rounding-point emulation (3 x its own distance from the reference;
tests/test_gemm_reference_cpu.py proves that every mutant lies at >= 3 x those bars).

Forms (svit_debug_set knobs; gemm_reference.FORMS): the heuristic, the v2 tiles cfg 0 / 2 / 4 at 2 / 3 / 4 stages and
K-steps of 32 / 64, the ring tiles cfg 5 / 6 / 7 at 2 / 3 / 4 stages (WAVE_PRIVATE epilogue, no workgroup barrier),
the one-round tiles cfg 9 / 10.  Every form takes
  * the whole epilogue list at 417 x 768 x 448 (partial last row tile of every tile height, partial 16-row slab):
    EPI_BF16, EPI_GELU with and without out2, EPI_DGELU, EPI_RESID without a scale and with rows_per_sample 20 / 54 /
    139 / 200 / 417, out of place and in place (which of them reads one scale per row and which two scales and a
    boundary per wave depends on the tile's wave height: gemm_reference.epilogue_list; 200 is the multi-sample case
    of the 160-row wave blocks), EPI_F32 plain, accumulate, remap, remap + accumulate;
  * EPI_F32 and EPI_BF16 at M = 1, 15, 130 and K = 32, 64 (K = 64 only where the form needs K % 64 == 0): one K-step
    under a 2- to 4-stage prologue, nk = 1 < STAGES on the ring (the loader issues min(STAGES, nk) tiles and both
    sides pass exactly nk barriers: gemm_nt_ring_kernel / nt_ring_loader), fewer rows than a 16-row slab.
The heuristic also takes the list at 417 x 384 x 96 and 130 x 384 x 2304 (its long-K choice).

Stride paths: every launch runs on contiguous outputs ("wide": 16-byte stores of 8 bf16 columns), with ldo = ldo2 =
ldaux = N + 4 ("col4": the 4-column stores), with N + 8 ("wide_gap") and, where out2 or aux has a stride of its own,
with only that one or only ldo at N + 4 ("col4_by_aux", "col4_by_out": either alone must select the 4-column path,
and a stride taken from the wrong tensor shows); `a` is always a column slice of a wider matrix.  All paths must
agree BIT for bit (same accumulators, same arithmetic); tile forms are not compared with each
other.  Every output is a view into a buffer pre-filled with a sentinel: 16 rows past M, the columns [N, ldo) and
the rows outside a remap window must come back untouched.

Each test prints one line per (form, epilogue, stride path, output): the worst metric / bar of the launch.

That the knobs of a form select the kernel it is named after -- and not, silently, another tile because N or K does
not fit -- is checked on the CPU: tests/test_gemm_nt_plan_cpu.py asks svit_debug_gemm_nt_plan (the chooser the launch
itself calls) at every shape a form is given; tests/test_gemm_reference_cpu.py asserts the N and K preconditions kept
in gemm_reference.FORMS.
"""
import ctypes as C

import pytest
import torch

from tests import gemm_reference as G

pytestmark = pytest.mark.gpu

DEV = "cuda"
# (name, columns beyond N of out, of out2 / aux); the mixed paths only where a second tensor has a stride of its own
PATHS = (("wide", 0, 0), ("col4", 4, 4), ("wide_gap", 8, 8), ("col4_by_aux", 0, 4), ("col4_by_out", 4, 0))
GUARD_ROWS = 16


@pytest.fixture(scope="module")
def lib():
    from svit_amd import hip
    return hip.load()


def _set_form(lib, form):
    f = G.FORMS[form]
    assert lib.svit_debug_set(0, f["stages"]) == 0 and lib.svit_debug_set(1, f["cfg"]) == 0
    assert lib.svit_debug_set(2, f["bk"]) == 0


def _launch(case, pad, pad2):
    """one svit_gemm_nt call of `case` with ldo = N + pad and ldo2 = ldaux = N + pad2.
    -> {tensor: (whole buffer on the CPU, expected buffer outside the written elements, destination rows)}."""
    from svit_amd import hip
    M, N, K = case.shape
    x = G.inputs(M, N, K)
    ld, ld2 = N + pad, N + (pad if case.inplace else pad2)
    a_wide = torch.full((M, K + 16), 3.0, dtype=G.BF16)
    a_wide[:, 8:8 + K] = x["a"]
    a_wide = a_wide.to(DEV)
    a = a_wide[:, 8:8 + K]                                           # lda = K + 16, 16-byte aligned
    w = x["w"].to(DEV)
    odt = G.BF16 if case.out_bf16 else G.F32
    dest = G.remap_rows(M, case.remap) if case.remap else torch.arange(M)
    rows = (G.remap_buffer_rows(M, case.remap) if case.remap else M) + GUARD_ROWS
    before = torch.full((rows, ld), G.SENTINEL, dtype=odt)
    if case.acc:
        ob = G.old_buffer(case)
        before[:ob.shape[0], :N] = ob
    if case.inplace:
        before[:M, :N] = x["aux32"]
    out = before.to(DEV)
    g = hip.GemmArgs()
    g.A, g.lda, g.W, g.ldw = a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0)
    bias = None if case.epi == "dgelu" else x["bias"].to(DEV)
    g.bias = hip.ptr(bias)
    g.out, g.ldo = out.data_ptr(), ld
    bufs = {"out": (out, before)}
    aux = None
    if case.epi == "gelu" and case.save:
        before2 = torch.full((M + GUARD_ROWS, ld2), G.SENTINEL, dtype=G.BF16)
        out2 = before2.to(DEV)
        g.out2, g.ldo2 = out2.data_ptr(), ld2
        bufs["out2"] = (out2, before2)
    if case.epi in ("resid", "dgelu"):
        aux = out if case.inplace else G.aux_buffer(case, pad2).to(DEV)
        g.aux, g.ldaux = aux.data_ptr(), ld2
    rs = None
    if case.rps:
        rs = G.row_scale_of(case).to(DEV)
        g.row_scale, g.rows_per_sample = rs.data_ptr(), case.rps
    g.M, g.N, g.K = M, N, K
    g.epilogue = {"bf16": hip.EPI_BF16, "gelu": hip.EPI_GELU, "resid": hip.EPI_RESID, "f32": hip.EPI_F32,
                  "dgelu": hip.EPI_DGELU}[case.epi]
    g.accumulate = int(case.acc)
    if case.remap:
        g.remap_L, g.remap_N, g.remap_off = case.remap
    hip.call("svit_gemm_nt", C.byref(g))
    torch.cuda.synchronize()
    del aux, rs, bias
    return {t: (o.cpu(), b, dest) for t, (o, b) in bufs.items()}


def _check(form, case, lines):
    """all stride paths of one case under the form that is set: canaries, bars, bit equality between the paths."""
    bars = G.case_bars(case.name)
    first = None
    failures = []
    second = (case.epi == "gelu" and case.save) or (case.epi in ("resid", "dgelu") and not case.inplace)
    for path, pad, pad2 in PATHS:
        if pad != pad2 and not second:
            continue
        res = _launch(case, pad, pad2)
        got = {}
        for t, (buf, before, dest) in res.items():
            got[t] = buf[dest, :case.N]
            # everything but the written elements is bit-identical to what the buffer held
            untouched = buf.clone()
            untouched[dest, :case.N] = before[dest, :case.N]
            assert torch.equal(untouched.view(torch.int16 if case.out_bf16 else torch.int32),
                               before.view(torch.int16 if case.out_bf16 else torch.int32)), \
                "%s %s %s %s: wrote outside the output" % (form, case.name, path, t)
            assert bool(torch.isfinite(got[t].float()).all()), (form, case.name, path, t)
            m, (r, c) = G.metric(case, t, got[t])
            line = "parity: %s %s %s %s %.3f  (metric %.3g / bar %.3g, worst at row %d col %d)" % (
                form, case.name, path, t, m / bars[t], m, bars[t], r, c)
            lines.append(line)
            if m > bars[t]:
                failures.append(line)
        if first is None:
            first = got
        else:
            for t in got:
                assert torch.equal(got[t], first[t]), \
                    "%s %s: the %s path differs from the wide path in %s" % (form, case.name, path, t)
    return failures


def _run(lib, form, shape, lst):
    lines, failures = [], []
    try:
        _set_form(lib, form)
        for kw in lst:
            failures += _check(form, G.case_of(shape, kw), lines)
    finally:
        lib.svit_debug_reset()
        print("\n".join(lines))
    assert not failures, "\n" + "\n".join(failures)


def _main_params():
    out = []
    for form in G.FORMS:
        for shape, lst in G.form_shapes(form):
            if lst is not G.SMALL_LIST:
                out.append(pytest.param(form, shape, id="%s-%dx%dx%d" % ((form,) + shape)))
    return out


@pytest.mark.parametrize("form,shape", _main_params())
def test_every_epilogue_of_a_form(lib, form, shape):
    _run(lib, form, shape, G.epilogue_list(shape[0]))


@pytest.mark.parametrize("form", list(G.FORMS))
def test_short_k_and_few_rows(lib, form):
    for shape, lst in G.form_shapes(form):
        if lst is G.SMALL_LIST:
            _run(lib, form, shape, lst)
