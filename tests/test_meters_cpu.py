"""svit_amd/meters.py without a GPU: on a CPU `device` the push is plain torch indexing, everything behind it -- the
ring, the one read per period, the host meters, the gloo merge -- is the code the GPU path runs.  Every logged number is
compared with `==` against tests/golden/meters.json, recorded from the reference's own meters
(tools/gen_meters_golden.py)."""
import ctypes
import json
import math
import os
import socket
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMING = ("time_diff", "eta", "mem", "gpu_mem", "RAM")


def dec(v):
    if isinstance(v, dict):
        if set(v) == {"f"}:
            return float.fromhex(v["f"])
        return {k: dec(x) for k, x in v.items()}
    if isinstance(v, list):
        return [dec(x) for x in v]
    return v


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "meters.json")) as f:
        return dec(json.load(f))


def cfg_for(period, num_classes=174, max_epoch=50):
    from svit_amd import config
    cfg = config.ssv2_cfg(4, 64)
    cfg.LOG_PERIOD = period
    cfg.MODEL.NUM_CLASSES = num_classes
    assert cfg.SOLVER.MAX_EPOCH == max_epoch
    return cfg


def numbers(stats):
    """a logged dict as the fixture holds it: without the wall-clock / memory fields, numpy scalars as Python floats"""
    if stats is None:
        return []
    return [{k: (float(v) if isinstance(v, float) else v) for k, v in stats.items() if k not in TIMING}]


def f32(v):
    return torch.tensor(v, dtype=torch.float64).to(torch.float32)


def test_scalar_meter(golden):
    from svit_amd.meters import ScalarMeter
    g = golden["scalar"]
    m = ScalarMeter(g["window"])
    for v, want in zip(g["values"], g["median_avg_global"]):
        m.add_value(v)
        assert [float(m.get_win_median()), float(m.get_win_avg()), float(m.get_global_avg())] == want
    m.reset()
    assert m.count == 0 and m.total == 0.0 and len(m.deque) == 0


@pytest.mark.parametrize("period", [1, 3, 10])
def test_train_meter_against_the_reference(golden, period):
    """2 1/2 periods and a second epoch behind reset(): iteration lines (None off-period) and epoch lines"""
    from svit_amd.meters import TrainMeter
    case = next(c for c in golden["train"] if c["period"] == period)
    meter = TrainMeter(case["epoch_iters"], cfg_for(period, max_epoch=case["max_epoch"]), device="cpu")
    seen = 0
    for epoch, ep in enumerate(case["epochs"]):
        vals = f32(ep["values"])
        for i in range(case["epoch_iters"]):
            meter.update_stats(ep["lrs"][i], ep["mb_size"], dloss={k: vals[i, j] for j, k in enumerate(case["keys"])})
            got = meter.log_iter_stats(epoch, i)
            assert (got is None) == ((i + 1) % period != 0)
            assert numbers(got) == ep["iter_lines"][i], (epoch, i)
            seen += got is not None
        assert numbers(meter.log_epoch_stats(epoch)) == ep["epoch_line"], epoch
        assert meter.num_samples == ep["mb_size"] * case["epoch_iters"]
        meter.reset()
        assert int(meter.state[0]) == 0 and meter.num_samples == 0
    assert seen == 2 * (case["epoch_iters"] // period)


@pytest.mark.parametrize("num_classes", [5, 174])
def test_val_meter_against_the_reference(golden, num_classes):
    """five batches, the last one short; NUM_CLASSES 5 takes ks = (1, 1); min_top1_err survives the reset"""
    from svit_amd.meters import ValMeter
    case = next(c for c in golden["val"] if c["num_classes"] == num_classes)
    meter = ValMeter(case["max_iter"], cfg_for(case["period"], num_classes, case["max_epoch"]), device="cpu")
    assert meter.ks == ((1, 5) if num_classes > 5 else (1, 1))
    for n, b in enumerate(case["batches"]):
        epoch, i = b["epoch"], n % case["max_iter"]
        logits, labels = f32(b["logits"]), torch.tensor(b["labels"])
        extra = f32(b["extra"])
        meter.update_stats(logits, labels, logits.shape[0], extra_metrices=dict(zip(case["extra_keys"], extra)))
        r = (int(meter.state[0]) - 1) % case["period"]
        assert meter.ring[r, -2:].tolist() == b["correct"]          # the counts are metrics.topks_correct's
        assert numbers(meter.log_iter_stats(epoch, i)) == case["iter_lines"][n], n
        if i == case["max_iter"] - 1:
            assert numbers(meter.log_epoch_stats(epoch)) == case["epoch_lines"][epoch]
            meter.reset()
    assert [len(b["labels"]) for b in case["batches"][:5]] == [4, 4, 4, 4, 3]


def test_bad_labels_and_ties_on_the_cpu_push():
    from svit_amd.meters import ValMeter
    meter = ValMeter(2, cfg_for(2, 8), device="cpu")
    logits = torch.zeros(4, 8)                                        # all scores equal: the lower index is ahead
    meter.update_stats(logits, torch.tensor([0, 4, 5, 7]), 4)
    assert meter.ring[0].tolist() == [1.0, 2.0]                       # rank 0 | ranks 0 and 4
    meter.update_stats(logits, torch.tensor([0, -1, 8, 4]), 4)
    assert meter.ring[1].tolist() == [1.0, 2.0] and meter.state.tolist() == [2, 2]
    assert meter.log_iter_stats(0, 0) is None
    got = meter.log_iter_stats(0, 1)
    assert got["top1_err"] == 75.0 and got["top5_err"] == 50.0
    assert meter.log_epoch_stats(0)["bad_labels"] == 2


def test_errors_are_raised_not_hidden():
    from svit_amd.meters import TrainMeter
    cfg = cfg_for(3)
    meter = TrainMeter(10, cfg, device="cpu")
    one = torch.tensor(1.0)
    for i in range(4):                                                # four pushes, no read: the ring of 3 overran
        meter.update_stats(1e-3, 2, dloss={"loss": one})
    with pytest.raises(RuntimeError, match="log_iter_stats must be called every iteration"):
        meter.log_iter_stats(0, 5)
    meter = TrainMeter(10, cfg, device="cpu")
    meter.update_stats(1e-3, 2, dloss={"loss_ce": one, "loss": one})
    with pytest.raises(ValueError, match="fixed by the first update"):
        meter.update_stats(1e-3, 2, dloss={"loss": one})
    meter.update_stats(1e-3, 2, dloss={"loss_ce": one, "loss": torch.tensor(float("nan"))})
    meter.update_stats(1e-3, 2, dloss={"loss_ce": one, "loss": one})
    with pytest.raises(RuntimeError, match=r"Got NaN losses.*first at iteration 1 "):
        meter.log_iter_stats(0, 2)
    meter = TrainMeter(10, cfg, device="cpu")
    with pytest.raises(ValueError, match="at most 16"):
        meter.update_stats(1e-3, 2, dloss={"l%d" % i: one for i in range(17)})
    # a NaN in an entry other than "loss" is a number to log, as in the reference
    meter = TrainMeter(10, cfg_for(1), device="cpu")
    meter.update_stats(1e-3, 2, dloss={"aux": torch.tensor(float("nan")), "loss": one})
    assert math.isnan(meter.log_iter_stats(0, 0)["aux"])


def test_header_binding_and_argument_checks():
    """hip.EXPORTS equals the header's list and names the new entry point; its refusals come before any launch (no
    GPU here, so a launch would fail differently)"""
    from svit_amd import hip
    from tests.test_abi import header_functions
    assert header_functions() == list(hip.EXPORTS) and "svit_meter_push" in hip.EXPORTS
    import __graft_entry__
    __graft_entry__.build()
    lib = hip.load()
    ptrs = (ctypes.c_void_p * 17)(*([16] * 17))
    ok = dict(ring=16, W=3, K=4, state=16, scalars=ptrs, ns=2, logits=16, labels=16, N=2, C=5, k0=1, k1=5)

    def rc(**kw):
        a = dict(ok, **kw)
        return lib.svit_meter_push(a["ring"], a["W"], a["K"], a["state"], a["scalars"], a["ns"], a["logits"],
                                   a["labels"], a["N"], a["C"], a["k0"], a["k1"], None)
    ARG, SHAPE = -4, -2
    assert rc(ring=None) == ARG and rc(state=None) == ARG and rc(scalars=None) == ARG and rc(labels=None) == ARG
    assert rc(scalars=(ctypes.c_void_p * 2)(16, None)) == ARG
    assert rc(W=0) == SHAPE and rc(W=-1) == SHAPE
    assert rc(K=2) == SHAPE and rc(K=5) == SHAPE and rc(logits=None, labels=None, K=4) == SHAPE
    assert rc(ns=17, K=19) == SHAPE
    assert rc(N=0) == SHAPE and rc(C=0) == SHAPE
    assert rc(k0=0) == SHAPE and rc(k1=6) == SHAPE and rc(k0=6) == SHAPE and rc(k1=0) == SHAPE


# ------------------------------------------------------------------------------------------------ gloo, two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    from svit_amd.meters import TrainMeter, ValMeter
    with open(os.path.join(ROOT, "tests", "golden", "meters.json")) as f:
        case = dec(json.load(f))["two_rank"]
    meter = TrainMeter(case["epoch_iters"], cfg_for(case["period"], max_epoch=case["max_epoch"]), device="cpu")
    vals, keys = f32(case["values"][rank]), case["keys"][rank]
    lines = []
    for i in range(case["epoch_iters"]):
        meter.update_stats(case["lrs"][i], case["mb_size"], dloss={k: vals[i, j] for j, k in enumerate(keys)})
        lines.append(numbers(meter.log_iter_stats(0, i)))
    epoch_line = numbers(meter.log_epoch_stats(0))
    # validation: different batch sizes and hits on the two ranks
    vm = ValMeter(2, cfg_for(2, 8), device="cpu")
    logits = torch.arange(8.0).repeat(3 + rank, 1)                   # class 7 first, then 6, ...
    labels = torch.tensor([7, 3, 0, 5][:3 + rank]) if rank else torch.tensor([7, 7, 3])
    for i in range(2):
        vm.update_stats(logits, labels, 7, extra_metrices={"loss": torch.tensor(0.1 + rank)})
        val_line = vm.log_iter_stats(0, i)
    torch.save({"lines": lines, "epoch_line": epoch_line, "val": numbers(val_line)}, out % rank)
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_merge_over_gloo(golden, tmp_path):
    """a video rank and an image rank (different keys): every rank logs the reference's merged lines"""
    import numpy as np
    import torch.multiprocessing as mp
    port, out = _free_port(), str(tmp_path / "rank%d.pt")
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_worker, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    case = golden["two_rank"]
    f = np.float32
    # du.all_reduce on the fp32 errors: rank 0 has 2 of 3 right at k = 1 (3 of 3 at k = 5), rank 1 1 of 4 (3 of 4)
    top1 = float(f(f((f(1) - f(2) / f(3)) * f(100)) + f((f(1) - f(1) / f(4)) * f(100))) * f(0.5))
    top5 = float(f(f((f(1) - f(3) / f(3)) * f(100)) + f((f(1) - f(3) / f(4)) * f(100))) * f(0.5))
    loss = float(f(f(f(0.1)) + f(1.1)) * f(0.5))
    for r in range(2):
        got = torch.load(out % r)
        assert got["lines"] == case["iter_lines"], r
        assert got["epoch_line"] == case["epoch_line"], r
        assert got["val"] == [{"_type": "val_iter", "epoch": "1/50", "iter": "2/2", "top1_err": top1, "top5_err": top5,
                               "extra_meter_loss": loss}], r
