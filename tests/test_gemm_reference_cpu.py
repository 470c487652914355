"""The measure of tests/test_gemm_parity_gpu.py has teeth -- proved on the CPU, without looking at a kernel.

For every case of the GPU test (a shape and an epilogue variant of svit_gemm_nt) the rounding-point emulation of
tests/gemm_reference.py gives the `floor` of every output under the per-element metric of that module; the GPU bar
is 3 x floor.  Every applicable mutant -- the float64 reference with one plausible kernel bug -- has to lie at
>= 3 x bar in at least one output of the case: an order of magnitude between "correct" and "wrong".  No mutant may
go without a case that rejects it.  The suite's older measure (max |got - ref| / max |ref| against 1.5e-2 / 1e-3,
tests/test_kernels_gpu.py) is shown to ACCEPT the tanh GELU, the GELU' mutants and the double rounding: the gap
this file and the GPU test close."""
import functools

import pytest
import torch

from tests import gemm_reference as G

F64 = torch.float64
GAP = 3.0                      # a mutant sits at >= GAP x bar = GAP x BAR_FACTOR x floor


@functools.lru_cache(maxsize=None)
def mutant_ratios(name):
    """{mutant: (metric / bar, tensor, (row, col))}: the best output of the case for every applicable mutant."""
    case = G.CASE_BY_NAME[name]
    bars = G.case_bars(name)
    out = {}
    for m in G.MUTANTS:
        if G.mutant_applies(m, case):
            got = G.reference(case, m)
            out[m] = max((G.metric(case, t, got[t])[0] / bars[t], t, G.metric(case, t, got[t])[1]) for t in case.tensors)
    return out


@pytest.mark.parametrize("name", [c.name for c in G.CASES])
def test_every_applicable_mutant_lies_far_above_the_bar(name, record_property):
    case = G.CASE_BY_NAME[name]
    floors = G.case_floors(name)
    record_property("floors", {t: "%.3g" % f for t, f in floors.items()})
    assert set(floors) == set(case.tensors)
    # the emulation lies under the bar by construction (bar = 3 x its own metric, at least 3 u); its metric is a few
    # fp32 roundings relative to S -- were it larger, S would not be the scale of the error and 3 x floor no bar
    emu = G.emulate(case)
    for t in case.tensors:
        m = G.metric(case, t, emu[t])[0]
        assert m <= floors[t] < G.BAR_FACTOR * floors[t] and G.U32 <= floors[t] < 16 * G.U32, (t, m, floors[t])
    # the float64 reference itself, rounded once where the kernel rounds, costs nothing under the metric
    ref = G.reference(case)
    for t in case.tensors:
        once = ref[t].to(torch.float32).to(torch.bfloat16 if case.out_bf16 else torch.float32)
        assert G.metric(case, t, once)[0] < G.U32, t
    ratios = mutant_ratios(name)
    assert set(ratios) == {m for m in G.MUTANTS if G.mutant_applies(m, case)} and len(ratios) >= 4
    for m, (top, t, where) in ratios.items():
        record_property(m, "%.1f x bar (%s at %s)" % (top, t, where))
        if m in G.NO_EXCEPTIONS:
            continue
        assert top >= GAP, "%s: mutant %s reaches only %.2f x bar (%s at %s)" % (case, m, top, t, where)


def test_every_mutant_is_rejected_by_some_case():
    seen = set()
    for c in G.CASES:
        seen |= {m for m, r in mutant_ratios(c.name).items() if r[0] >= GAP}
    assert seen == set(G.MUTANTS) - set(G.NO_EXCEPTIONS)
    assert len(G.NO_EXCEPTIONS) <= 2 and len(G.MUTANTS) >= 16


def test_cases_name_every_path():
    """shapes, forms and epilogue variants the GPU test is asked to run."""
    assert {c.M for c in G.CASES} == {1, 15, 130, 417}
    assert {c.N for c in G.CASES} == {96, 192, 384, 768}
    assert {c.K for c in G.CASES} == {32, 64, 96, 448, 2304}
    assert (130, 384, 2304) in {c.shape for c in G.CASES}
    cfgs = {(f["cfg"], f["stages"], f["bk"]) for f in G.FORMS.values()}
    assert cfgs >= {(c, s, b) for c in (0, 2, 4) for s in (2, 3, 4) for b in (32, 64)}
    assert cfgs >= {(c, s, 0) for c in (5, 6, 7) for s in (2, 3, 4)} | {(-1, 0, 0), (9, 0, 0), (10, 0, 0)}
    for form, f in G.FORMS.items():
        shapes = G.form_shapes(form)
        (M, N, K), lst = shapes[0]
        assert (M, N, K) == (417, 768, 448) and K % 64 == 0 and N % 256 == 0 and N % 192 == 0 and N % 128 == 0
        variants = {G.case_of((M, N, K), kw).variant for kw in lst}
        assert variants >= {"bf16", "gelu", "gelu_nosave", "dgelu", "resid_noscale", "f32", "f32_acc", "f32_remap",
                            "f32_remap_acc"}
        for rps in (20, 54, 139, 200, 417):
            assert {"resid_rps%d" % rps, "resid_rps%d_inplace" % rps} <= variants
        # both ways of reading the row scale, each where a wrong one shows: a rows_per_sample below 32 RB (per-row)
        # and one at or above it (two scales and a boundary per wave) with SEVERAL samples whose boundaries fall
        # inside wave blocks of 32 RB rows, and the row-scale mutants proved on exactly those cases
        rb = f["rb"]
        multi = [kw["rps"] for kw in lst if kw["epi"] == "resid" and 0 < kw.get("rps", 0) < M]
        assert any(r < 32 * rb for r in multi), form
        fast = [r for r in multi if r >= 32 * rb]
        assert fast, form
        for r in fast:
            inside = [b for b in range(r, M, r) if b % (32 * rb)]
            assert inside, (form, r)
            scales = G.row_scale_of(G.case_of((M, N, K), dict(epi="resid", rps=r)))
            assert all(float(scales[i]) != float(scales[i + 1]) for i in range(len(scales) - 1))
            for inplace in (False, True):
                c = G.case_of((M, N, K), dict(epi="resid", rps=r, inplace=inplace))
                got = mutant_ratios(c.name)
                assert all(got[m][0] >= GAP for m in ("rs_first_row", "rs_boundary_off1", "rs_div_plus1")), (form, r)
        small = [(s, l) for s, l in shapes if l is G.SMALL_LIST]
        assert {s[0] for s, _ in small} >= {1, 15} and {s[2] for s, _ in small} == ({64} if f["k64"] else {32, 64})
        for (m, n, k), l in small:
            assert {kw["epi"] for kw in l} == {"f32", "bf16"}
            assert n % {0: 192, 4: 128, 9: 256, 10: 192}.get(f["cfg"], 96) == 0
            assert not (f["k64"] and k % 64)
    # the heuristic's K-step-64 shortcut and its long-K choice
    M, N, K = G.MAIN_SHAPE
    assert K % 64 == 0 and N <= 768 and K >= 384
    assert {f["rb"] for f in G.FORMS.values()} == {1, 2, 3, 5}
    assert [r for r in (20, 54, 139, 200) if r >= 160] == [200]      # the one multi-sample rs_fast case of RB = 5
    # the remap leaves rows outside its window
    L, ntok, off = G.remap_of(417)
    assert 417 % L == 0 and ntok > L + off and G.remap_buffer_rows(417, (L, ntok, off)) == 3 * ntok
    rows = G.remap_rows(417, (L, ntok, off))
    assert len(set(rows.tolist())) == 417 and int(rows.max()) < 3 * ntok


def test_inputs_reach_the_tails_and_the_neighbourhood_of_zero():
    case = G.CASE_BY_NAME["417x768x448-gelu"]
    acc, bias, S = G.terms(case)
    h = acc + bias
    assert float(h.min()) < -6 and float(h.max()) > 6
    assert int((h.abs() < G.SMALL_X).sum()) >= 100                   # where gelu' = 1/2 + x pdf(x) needs its second term
    assert int(((h > -6.5) & (h < -4)).sum()) >= 100                 # the lower tail: |gelu| < 1e-4
    rs = G.row_scale_of(G.CASE_BY_NAME["417x768x448-resid_rps20"])
    assert len(rs) == 21 and all(float(rs[i]) != float(rs[i + 1]) for i in range(20))
    assert float(G.inputs(417, 768, 448)["bias"].abs().max()) > 0.45


def test_reference_gelu_is_autograd_and_the_emulated_erf_is_the_documented_one():
    x = torch.linspace(-9, 9, 4001, dtype=F64, requires_grad=True)
    y = torch.nn.functional.gelu(x)
    (g,) = torch.autograd.grad(y.sum(), x, create_graph=True)
    (g2,) = torch.autograd.grad(g.sum(), x)
    xd = x.detach()
    assert float((G.gelu64(xd) - y.detach()).abs().max()) < 1e-14
    assert float((G.dgelu64(xd) - g.detach()).abs().max()) < 1e-14
    assert float((G.d2gelu64(xd) - g2).abs().max()) < 1e-13
    assert float(G.d2gelu64(xd).abs().max()) < 1.0                   # C2 of the derivative bound
    e, d = G.gelu_parts32(xd.float())
    # Abramowitz-Stegun 7.1.26: |erf error| <= 1.5e-7 -> gelu within |x| 0.75e-7 and a little fp32 arithmetic
    assert float((e.double() - G.gelu64(xd)).abs().max()) < 1.5e-6
    ag, ad = G.abs_terms()
    assert 5e-8 < ag < 1e-6 and 5e-8 < ad < 2e-6
    # the tanh form is up to 5e-4 away: three orders of magnitude above the absolute term
    assert 1e-4 < float((G.gelu_tanh64(xd) - G.gelu64(xd)).abs().max()) < 1e-3


@pytest.mark.parametrize("mutant,name", [("gelu_tanh", "417x768x448-gelu"), ("dgelu_no_xpdf", "417x768x448-gelu"),
                                         ("dgelu_at_bf16_h", "417x768x448-gelu"), ("double_round", "417x768x448-bf16"),
                                         ("double_round", "417x768x448-dgelu")])
def test_old_measure_accepts_these_mutants(mutant, name):
    """The gap: max |got - ref| / max |ref| < 1.5e-2 (what tests/test_kernels_gpu.py asserts of a bf16 output)
    accepts the tanh approximation, a gelu' without x.pdf near 0, a gelu' of the rounded h and a second rounding;
    the per-element metric rejects each by more than an order of magnitude."""
    case = G.CASE_BY_NAME[name]
    ref, got = G.reference(case), G.reference(case, mutant)
    for t in case.tensors:
        assert G.old_measure(got[t], ref[t]) < G.OLD_BAR_BF16, (t, G.old_measure(got[t], ref[t]))
    top, t, where = mutant_ratios(name)[mutant]
    assert top >= 10 * GAP, (mutant, top, t, where)


def test_old_measure_accepts_a_wrong_group_in_a_small_element():
    """a wrong fp32 value in one 4-column group of one row, of the size of a typical element: invisible at 1e-3 of the
    largest element unless that element is large; 10^4 bars under the per-element metric."""
    case = G.CASE_BY_NAME["417x768x448-f32"]
    ref = G.reference(case)["out"]
    got = ref.clone()
    r = 6                                                            # a row of gain 0.01: |h| ~ |bias|
    got[r, 100:104] += 5e-4 * ref.abs().max()                        # half the old bar: several times the element itself
    assert float(ref[r].abs().max()) < 1.0 < float(ref.abs().max())
    assert G.old_measure(got, ref) < G.OLD_BAR_F32
    assert G.metric(case, "out", got)[0] >= 100 * G.case_bars(case.name)["out"]
