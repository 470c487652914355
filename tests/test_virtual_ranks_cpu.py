"""Virtual ranks without a GPU: which recipe ranks a real rank runs (dp.virtual_roles on the reference's own
configs/ssv2.yaml, tests/golden/ssv2.yaml) and the meter's merge over the rings of the virtual ranks
(meters.TrainMeter(virtual_ranks=k) on the CPU branch of the push: everything behind the push is the code the GPU path
runs)."""
import os

import pytest
import torch

from svit_amd import config, dp


@pytest.fixture(scope="module")
def recipe(golden_dir):
    cfg = config.get_cfg()
    cfg.merge_from_file(os.path.join(golden_dir, "ssv2.yaml"))
    assert cfg.NUM_GPUS == 8 and list(cfg.IMAGE_TRAIN.GPU_IDS) == [7]
    return cfg


@pytest.mark.parametrize("world", [1, 2, 4, 8])
def test_virtual_roles_of_the_shipped_recipe(recipe, world):
    k = 8 // world
    seen = []
    for rank in range(world):
        roles = dp.virtual_roles(recipe, world, rank)
        assert len(roles) == k
        assert roles == [dp.rank_role(recipe, i) for i in range(rank * k, (rank + 1) * k)]     # the contiguous block
        # the image role (recipe rank 7) is the LAST entry of the LAST real rank and nowhere else
        assert [r.is_image for r in roles] == [False] * (k - 1) + [rank == world - 1]
        assert [r.batch_size for r in roles] == [63 if r.is_image else 9 for r in roles]
        assert [r.replicas for r in roles] == [1 if r.is_image else 7 for r in roles]
        seen += roles
    # all real ranks together: the eight recipe ranks once, in order; the loader shards as in the 8-rank job
    assert seen == [dp.rank_role(recipe, i) for i in range(8)]
    assert [r.data_rank for r in seen] == [0, 1, 2, 3, 4, 5, 6, 0]
    assert [r.dataset for r in seen] == [recipe.TRAIN.DATASET] * 7 + ["multi_images"]


def test_world_of_the_recipe_is_todays_single_role(recipe):
    for rank in range(8):
        assert dp.virtual_roles(recipe, 8, rank) == [dp.rank_role(recipe, rank)]


def test_virtual_roles_refusals(recipe):
    with pytest.raises(ValueError, match="divide"):
        dp.virtual_roles(recipe, 3, 0)
    with pytest.raises(ValueError, match="divide"):
        dp.virtual_roles(recipe, 16, 0)
    with pytest.raises(ValueError, match="divide"):
        dp.virtual_roles(recipe, 0, 0)
    for world, rank in ((2, 2), (2, -1), (1, 1), (8, 8)):
        with pytest.raises(ValueError, match="outside"):
            dp.virtual_roles(recipe, world, rank)


# ------------------------------------------------------------------------------------------------ the meter ----
VIDEO = ("loss_ce", "loss")
IMAGE = ("boxes_l1_loss", "boxes_bce_loss", "loss")


def _cfg(period):
    cfg = config.ssv2_cfg(4, 64)
    cfg.LOG_PERIOD = period
    return cfg


def _val(it, vrank, j):
    """fp32 values with full mantissas (so that a merge in fp32 instead of Python doubles would show)"""
    return torch.tensor(0.3 + 0.173 * it + 1.37 * vrank + 0.0711 * j, dtype=torch.float64).to(torch.float32)


def test_meter_merges_virtual_ranks_per_key():
    """two virtual ranks with different key sets, three iterations, LOG_PERIOD = 3: per key the mean in Python doubles
    over the ranks that have the key, the median of the window, the epoch's global average; mb_size summed once"""
    import numpy as np
    from svit_amd.meters import TrainMeter
    meter = TrainMeter(3, _cfg(3), device="cpu", virtual_ranks=2)
    rows = []
    for it in range(3):
        v = {k: _val(it, 0, j) for j, k in enumerate(VIDEO)}
        im = {k: _val(it, 1, j) for j, k in enumerate(IMAGE)}
        meter.push(v, vrank=0)
        meter.push(im, vrank=1)
        meter.host_update(1e-3 * (it + 1), 5)
        per_key = {}
        for d in (v, im):                                       # recipe-rank order
            for k, x in d.items():
                per_key.setdefault(k, []).append(float(x))
        rows.append({k: sum(x) / len(x) for k, x in per_key.items()})
        got = meter.log_iter_stats(0, it)
        assert (got is None) == (it < 2)
    assert set(rows[0]) == {"loss_ce", "loss", "boxes_l1_loss", "boxes_bce_loss"}
    for k in rows[0]:
        assert float(got[k]) == float(np.median([r[k] for r in rows])), k
    assert got["lr"] == 3e-3 and meter.num_samples == 15
    # the merged values the host meters were fed, one by one
    for k in rows[0]:
        assert list(meter.multi_loss.losses[k].deque) == [r[k] for r in rows], k
    # "loss" is the mean of both ranks, the other keys of the one rank that has them
    assert rows[1]["loss"] == (float(_val(1, 0, 1)) + float(_val(1, 1, 2))) / 2
    assert rows[1]["loss_ce"] == float(_val(1, 0, 0)) and rows[1]["boxes_bce_loss"] == float(_val(1, 1, 1))
    ep = meter.log_epoch_stats(0)
    for k in rows[0]:
        assert float(ep[k]) == sum(r[k] for r in rows) / 3, k
    meter.reset()
    assert meter.num_samples == 0 and all(int(r.state[0]) == 0 for r in meter._rings)


def test_meter_virtual_rank_interface_refusals():
    from svit_amd.meters import TrainMeter
    meter = TrainMeter(4, _cfg(2), device="cpu", virtual_ranks=2)
    one = {"loss": torch.tensor(1.0)}
    with pytest.raises(ValueError, match="vrank"):
        meter.push(one)
    with pytest.raises(ValueError, match="vrank"):
        meter.push(one, vrank=2)
    with pytest.raises(ValueError, match="virtual_ranks"):
        meter.update_stats(1e-3, 2, dloss=one)
    with pytest.raises(ValueError, match="without virtual_ranks"):
        TrainMeter(4, _cfg(2), device="cpu").push(one, vrank=0)
    # a virtual rank that pushed nothing this iteration is caught at the read
    meter.push(one, vrank=0)
    meter.push(one, vrank=1)
    meter.host_update(1e-3, 2)
    meter.push(one, vrank=0)
    meter.host_update(1e-3, 2)
    with pytest.raises(RuntimeError, match="pushed 1 iterations"):
        meter.log_iter_stats(0, 1)


def test_nan_names_iteration_and_virtual_rank():
    from svit_amd.meters import TrainMeter
    meter = TrainMeter(4, _cfg(2), device="cpu", virtual_ranks=2)
    for it in range(2):
        meter.push({"loss": torch.tensor(1.0)}, vrank=0)
        meter.push({"loss": torch.tensor(float("nan") if it == 1 else 2.0)}, vrank=1)
        meter.host_update(1e-3, 2)
    with pytest.raises(RuntimeError, match=r"iteration 1 of the epoch \(virtual rank 1\)"):
        meter.log_iter_stats(0, 1)


def test_meter_without_virtual_ranks_is_todays():
    """the buffer (4 int32 of state + W x K floats), its contents after a push and the drained row of a plain meter"""
    from svit_amd.meters import TrainMeter
    meter = TrainMeter(4, _cfg(3), device="cpu")
    assert meter.virtual_ranks is None and meter._rings is None
    vals = {k: _val(0, 0, j) for j, k in enumerate(IMAGE)}
    meter.update_stats(1e-3, 7, dloss=vals)
    assert meter.buf.dtype == torch.int32 and meter.buf.numel() == 4 + 3 * len(IMAGE)
    assert tuple(meter.ring.shape) == (3, len(IMAGE)) and int(meter.state[0]) == 1 and int(meter.state[1]) == 0
    assert meter.ring[0].tolist() == [float(v) for v in vals.values()] and not meter.ring[1:].any()
    drained = meter._drain()
    assert drained == [((1e-3, 7), [{k: float(v) for k, v in vals.items()}])]


# ----------------------------------------------------------------- two real ranks x two virtual ranks over gloo ----
def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _recipe_val(it, recipe_rank, j):
    return torch.tensor(0.3 + 0.173 * it + 1.37 * recipe_rank + 0.0711 * j, dtype=torch.float64).to(torch.float32)


def _gloo_worker(rank, world, port, out):
    import sys
    import numpy as np
    import torch.distributed as dist
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    from svit_amd.meters import TrainMeter
    gathers = []
    all_gather = dist.all_gather
    dist.all_gather = lambda parts, t, *a, **kw: (gathers.append(t.numel()), all_gather(parts, t, *a, **kw))[1]
    # recipe ranks 0..3 = (real rank, virtual rank) (0,0) (0,1) (1,0) (1,1); recipe rank 3 is the image rank
    keys = lambda recipe_rank: IMAGE if recipe_rank == 3 else VIDEO
    meter = TrainMeter(4, _cfg(2), device="cpu", virtual_ranks=2)

    def iteration(it):
        for v in range(2):
            rr = rank * 2 + v
            meter.push({k: _recipe_val(it, rr, j) for j, k in enumerate(keys(rr))}, vrank=v)
        meter.host_update(1e-3, 10)
    iteration(0)
    iteration(1)
    drained = meter._drain()                       # the rows of every iteration, in recipe-rank order on every rank
    assert len(gathers) == 1 and gathers[0] == 2 * (4 + 2 + 2 * 3)        # ONE gather: two rings padded to 3 columns
    want = [((1e-3, 10), [{k: float(_recipe_val(it, rr, j)) for j, k in enumerate(keys(rr))} for rr in range(4)])
            for it in range(2)]
    assert drained == want, (drained, want)
    iteration(2)
    assert meter.log_iter_stats(0, 2) is None
    iteration(3)
    got = meter.log_iter_stats(0, 3)
    assert len(gathers) == 2
    lines = []
    for it in (2, 3):
        per_key = {}
        for rr in range(4):
            for j, k in enumerate(keys(rr)):
                per_key.setdefault(k, []).append(float(_recipe_val(it, rr, j)))
        lines.append({k: sum(v) / len(v) for k, v in per_key.items()})
    assert set(lines[0]) == set(VIDEO) | set(IMAGE)
    for k in lines[0]:
        assert float(got[k]) == float(np.median([lines[0][k], lines[1][k]])), k
    assert meter.num_samples == 20
    torch.save(True, out % rank)
    dist.barrier()
    dist.destroy_process_group()


def test_virtual_ranks_across_two_real_ranks_over_gloo(tmp_path):
    import torch.multiprocessing as mp
    port, out = _free_port(), str(tmp_path / "rank%d.pt")
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    assert all(torch.load(out % r) for r in range(2))
