"""The yardstick of tests/test_pool_parity_gpu.py, proven on the CPU (no GPU needed): the float64 restatement of the pooled
q/k/v path is the oracle's, the rounding-point emulation sits inside its own bars, every mutant of
tests/pool_reference.py lies at >= 3 x bar in some output of some case, and the cases take the kernel forms and show the
chunk cuts they name (asked of ops.pool_plan, the chooser and chunk search the launches themselves call)."""
import pytest
import torch

from oracle import svit_ref as R
from tests import pool_reference as P

F64 = torch.float64
SEPARATION = 3.0          # a mutant counts where m >= SEPARATION x bar


@pytest.fixture(scope="module")
def host():
    import __graft_entry__
    __graft_entry__.build()
    from svit_amd import hip, ops
    return ops, hip.load()


@pytest.fixture(scope="module")
def plans(host):
    ops, lib = host
    return {c.name: P.plans_of(c, ops, lib) for c in P.CASES}


@pytest.mark.parametrize("name", ["stream-2x7x7-s122", "stream-2x30x23-s188", "frame-1x9x9-s222"])
def test_reference_restates_the_oracle(name):
    """reference_conv + reference_ln in float64 = oracle.svit_ref.pool_tokens (depthwise Conv3d, object gain, cls row,
    LayerNorm) evaluated in float64 on the same bf16 inputs and bf16-rounded weights"""
    c = P.CASE_BY_NAME[name]
    X = P.inputs(name)
    for i, s in enumerate(c.strides):
        w = P._b16(X["ws"][i])
        ga, be = X["gammas"][i].to(F64), X["betas"][i].to(F64)
        ref, thw_o = R.pool_tokens(P.x_of(c, i).to(F64), c.thw, (1, s, s), w.reshape(96, 1, 3, 3, 3), ga, be, c.n_obj)
        assert thw_o == (c.thw[0], c.Ho[i], c.Wo[i]) and ref.dtype == F64
        pre = P.reference_conv(c, i)
        rows = slice(0, 1 + c.Lo[i])              # (the kernels take g(w) from the fp32 weights: the object rows separately)
        mine = torch.nn.functional.layer_norm(pre, (96,), ga, be, P.EPS)
        assert float((mine[:, :, rows] - ref[:, :, rows]).abs().max()) < 1e-12
        g = R.object_gain(X["ws"][i].to(F64).reshape(96, 1, 3, 3, 3), (1, s, s))
        assert float((pre[:, :, 1 + c.Lo[i]:] - P.x_of(c, i).to(F64)[:, :, 1 + c.L:] * g).abs().max()) < 1e-15


@pytest.mark.parametrize("case", P.CASES, ids=lambda c: c.name)
def test_emulation_within_its_own_bar(case):
    chain, floors, bars = P.emulated_chain(case.name), P.case_floors(case.name), P.case_bars(case.name)
    for i in range(3):
        e = chain[i]
        ms = dict(P.check_conv(case, i, e["pre"]))
        ms.update(P.check_ln(case, i, e["pre"], e["out"], e["mean"], e["rstd"]))
        ms.update(P.check_ln_bwd(case, i, e["pre"], e["mean"], e["rstd"], e["dpre"], e["dgamma"], e["dbeta"]))
        ms.update(P.check_conv_bwd(case, i, e["dpre"], e["dqkv"], e["dw"]))
        print("%-22s %s floors  %s" % (case.name, "qkv"[i], "  ".join("%s %.2e" % (k, floors[i][k]) for k in P.OUTPUTS)))
        for k in P.OUTPUTS:
            assert P.U32 <= floors[i][k] and ms[k][0] <= floors[i][k] < bars[i][k], (i, k)
        # what the emulation stores also meets the exact demands of the GPU test
        assert torch.equal(e["dqkv"][:, :, 0], e["dpre"][:, :, 0])
        T, H, W = case.thw
        dx = e["dqkv"][:, :, 1:1 + case.L].reshape(case.B, case.heads, T, H, W, 96)
        assert float(dx[:, :, :, ~P.window_mask(case, i)].abs().max() if not P.window_mask(case, i).all() else 0.0) == 0.0


def _first_separation(mutant, plans):
    """-> (case, tensor, {output: ratio}, old-measure verdict, top ratio) of the first (smallest) case that separates the
    mutant, the best ratio seen otherwise; None where the mutant applies nowhere.  The verdict of the suite's whole-tensor
    measures is taken there and at the LARGEST case the mutant applies to (one wrong row weighs least in the largest
    tensor): the mutant counts as passed by them if either passes."""
    best = None
    order = sorted(P.CASES, key=lambda c: c.L * c.B * c.heads)
    largest = next(((c, i) for c in reversed(order) for i in range(3) if P.mutant_applies(mutant, c, i, plans[c.name])), None)
    if largest is None:
        return None
    old_large = P.old_measure_passes(P.mutant_outputs(largest[0], largest[1], mutant, plans[largest[0].name])[0])
    for case in order:
        bars = P.case_bars(case.name)
        for i in range(3):
            if not P.mutant_applies(mutant, case, i, plans[case.name]):
                continue
            pairs, ms = P.mutant_outputs(case, i, mutant, plans[case.name])
            ratios = {k: v / bars[i][k] for k, v in ms.items()}
            top = max(ratios.values())
            rec = (case.name, i, ratios, P.old_measure_passes(pairs) or old_large, top)
            if top >= SEPARATION:
                return rec
            if best is None or top > best[4]:
                best = rec
    return best


def test_mutants_separate(plans):
    """Every mutant lies at >= 3 x bar in at least one output of at least one case it applies to, and none applies to no
    case.  The report names, per mutant, the case and outputs that catch it and whether the suite's whole-tensor measures
    (tests/test_kernels_gpu.py: max |got - ref| / max |ref| and a cosine, at their tightest bars) would have passed it there."""
    passed_by_old, failed = [], []
    for mutant in P.MUTANTS:
        rec = _first_separation(mutant, plans)
        assert rec is not None, "%s applies to no case" % mutant
        name, i, ratios, old_ok, top = rec
        print("%-26s %-22s %s  m/bar: %s   whole-tensor measures: %s"
              % (mutant, name, "qkv"[i], "  ".join("%s %.3g" % kv for kv in ratios.items()), "PASS" if old_ok else "fail"))
        if old_ok:
            passed_by_old.append(mutant)
        if top < SEPARATION and mutant not in P.EXCEPTIONS:
            failed.append((mutant, top))
    print("the whole-tensor measures would have passed:", ", ".join(passed_by_old))
    assert not failed, failed
    assert len(P.EXCEPTIONS) <= 2 and not set(P.EXCEPTIONS) & set(P.BOUNDARY_MUTANTS)
    assert tuple(passed_by_old) == P.OLD_MEASURE_PASSES        # (the list the module's docstring carries)


def _cut_not_at_end(plan, i, extent):
    return plan is not None and plan["y_chunks"][i] >= 2 and 0 < plan["r_per"][i] < extent


def test_cases_cover_every_path_and_cut(plans):
    """every case takes the forward path it names under its knobs and shows the cuts it names; together the cases cover
    every forward path, a y-cut inside the plane per stride class and a t-cut of the staged forward and of the fused backward,
    a multi-chunk slab plan, a frame pass over several row bands, and every addend variant of the LayerNorm backward on a
    small and on a step-shaped Nout"""
    seen, variants = set(), set()
    for c in P.CASES:
        pl = plans[c.name]
        path, launches = pl["fwd"]
        assert path == c.path, (c.name, path)
        assert pl["bwd"] is not None, c.name                      # (the product library has no other conv backward)
        assert 3 * 27 * 96 * c.B * c.heads * pl["bwd"]["max_chunks"] > 0
        T, H, W = c.thw
        BH = c.B * c.heads
        have = set()
        for i, s in enumerate(c.strides):
            cls = min(s, 3)
            if pl["staged"] is not None:
                if _cut_not_at_end(pl["staged"], i, c.Ho[i]):
                    have.add("fy%d" % cls)
                if pl["staged"]["t_chunks"][i] >= 2:
                    have.add("ft")
            if _cut_not_at_end(pl["bwd"], i, P.unit_rows(s, H)):
                have.add("by%d" % cls)
            if pl["bwd"]["t_chunks"][i] >= 2:
                have.add("bt")
        if path in ("slab", "mfma") and launches[0][0] == "pool_slab_fwd" and launches[0][1] > BH * 12:
            have.add("slab")                                      # grid = chunks x batch*heads x 12
        if path == "frame" and launches[0][1] > 3 * BH:
            have.add("frame")                                     # at most one workgroup per item: some tensor has > BH items
        assert set(c.cuts) <= have, (c.name, sorted(set(c.cuts) - have))
        seen |= {(c.path, cut) for cut in c.cuts} | {(c.path, None)}
        for i in range(3):
            variants.add((c.lnb[i], "small" if c.Nout[i] <= 150 else "step" if c.Nout[i] >= 393 else "mid"))
    assert {p for p, _ in seen} == set(P.FORWARD_PATHS)
    for cut in ("fy1", "fy2", "fy3", "ft"):
        assert ("staged", cut) in seen, cut
    for cut in ("by1", "by2", "by3", "bt"):
        assert any(k == cut and p in ("staged", "slab", "mfma") for p, k in seen), cut      # (the issue: on the staged and slab shapes)
    assert ("slab", "slab") in seen and ("frame", "frame") in seen
    for v in P.LNB_VARIANTS:
        assert (v, "small") in variants and (v, "step") in variants, v
