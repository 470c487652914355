"""Record tests/golden/meters.json from the reference's own meters (TEST INFRASTRUCTURE, run where the reference
tree exists; nothing of it is copied: the file holds input sequences and the dicts its meters logged).

    python tools/gen_meters_golden.py

The reference's ScalarMeter / MultiLossMeter / TrainMeter / ValMeter (slowfast/utils/meters.py:401-709, 793-866) and
metrics.topks_correct / topk_errors (slowfast/utils/metrics.py:9-62) are loaded through oracle/ref_shim; modules the
image lacks get empty stand-ins here.  `logging.log_json_stats` is captured: what is recorded is the dict a meter hands
to it, without the wall-clock and memory fields.  Every float is written with float.hex.

Sequences: 2 1/2 periods (and a second epoch behind a reset) of a three-key loss dict at LOG_PERIOD 1, 3 and 10; a
two-rank run whose ranks log different keys, merged as tools/train_net.py:153-161 merges them; a validation epoch of five
batches, the last one short, at NUM_CLASSES 5 and 174.
"""
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "meters.json")
DROP = ("time_diff", "eta", "mem", "gpu_mem", "RAM")


class _Anything(types.ModuleType):
    """stand-in for a module the image lacks: every attribute is a callable that refuses to run"""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def absent(*a, **k):
            raise RuntimeError("%s.%s is a stand-in" % (self.__name__, name))
        return absent


def load_reference():
    from oracle import ref_shim
    ref_shim.install()
    for _ in range(32):
        try:
            meters = importlib.import_module("slowfast.utils.meters")
            break
        except ModuleNotFoundError as e:
            sys.modules[e.name] = _Anything(e.name)
    else:
        raise RuntimeError("the reference's meters do not import")
    import slowfast.utils.metrics as metrics
    logged = []
    meters.logging.log_json_stats = lambda stats: logged.append(dict(stats))
    meters.misc.gpu_mem_usage = lambda: 0.0
    meters.misc.cpu_mem_usage = lambda: (0.0, 0.0)
    return meters, metrics, logged


def enc(v):
    if isinstance(v, (float, np.floating)):
        return {"f": float(v).hex()}
    if isinstance(v, dict):
        return {k: enc(x) for k, x in v.items() if k not in DROP}
    if isinstance(v, (list, tuple)):
        return [enc(x) for x in v]
    if isinstance(v, (np.integer,)):
        return int(v)
    return v


def f32(rng, *shape):
    return rng.standard_normal(shape).astype(np.float32)


def cfg_for(period, num_classes=174):
    from oracle import ref_shim
    cfg = ref_shim.reference_cfg()
    cfg.LOG_PERIOD = period
    cfg.MODEL.NUM_CLASSES = num_classes
    return cfg


def take(logged):
    out = [enc(d) for d in logged]
    del logged[:]
    return out


def train_case(meters, logged, period, rng):
    keys = ["loss_ce", "video_image_desc_l2_loss", "loss"]
    iters = (5 * period + 1) // 2
    cfg = cfg_for(period)
    meter = meters.TrainMeter(iters, cfg)
    case = {"period": period, "epoch_iters": iters, "max_epoch": cfg.SOLVER.MAX_EPOCH, "keys": keys, "epochs": []}
    for epoch in range(2):
        vals = np.abs(f32(rng, iters, len(keys))) + np.float32(0.25)
        lrs = [float(1e-4 * (1 + i + epoch * iters)) for i in range(iters)]
        lines = []
        meter.iter_tic()
        for i in range(iters):
            meter.data_toc()
            meter.update_stats(lrs[i], 8, dloss={k: torch.tensor(vals[i, j]) for j, k in enumerate(keys)})
            meter.iter_toc()
            meter.log_iter_stats(epoch, i)
            lines.append(take(logged))
            meter.iter_tic()
        meter.log_epoch_stats(epoch)
        epoch_line = take(logged)
        meter.reset()
        case["epochs"].append({"values": enc(vals.tolist()), "lrs": enc(lrs), "mb_size": 8,
                               "iter_lines": lines, "epoch_line": epoch_line})
    return case


def two_rank_case(meters, logged, rng):
    """a video rank and an image rank: different keys, merged per iteration in rank order (train_net.py:153-161)"""
    period, iters = 3, 8
    keys = [["loss_ce", "video_image_desc_l2_loss", "loss"],
            ["boxes_l1_loss", "boxes_bce_loss", "boxes_giou_loss", "loss_contact_state", "loss"]]
    vals = [np.abs(f32(rng, iters, len(k))) + np.float32(0.25) for k in keys]
    cfg = cfg_for(period)
    meter = meters.TrainMeter(iters, cfg)
    lrs = [float(2e-4 * (1 + i)) for i in range(iters)]
    lines = []
    for i in range(iters):
        gathered = [{k: torch.tensor(vals[r][i, j]).item() for j, k in enumerate(keys[r])} for r in range(2)]
        merged = {}
        for d in gathered:
            for k, v in d.items():
                merged.setdefault(k, []).append(v)
        merged = {k: sum(v) / len(v) for k, v in merged.items()}
        meter.update_stats(lrs[i], 2 * 2, dloss=merged)
        meter.log_iter_stats(0, i)
        lines.append(take(logged))
    meter.log_epoch_stats(0)
    return {"period": period, "epoch_iters": iters, "max_epoch": cfg.SOLVER.MAX_EPOCH, "keys": keys,
            "values": [enc(v.tolist()) for v in vals], "lrs": enc(lrs), "mb_size": 4, "iter_lines": lines,
            "epoch_line": take(logged)}


def val_case(meters, metrics, logged, num_classes, rng):
    period, sizes = 2, [4, 4, 4, 4, 3]
    cfg = cfg_for(period, num_classes)
    meter = meters.ValMeter(len(sizes), cfg)
    ks = (1, 5) if num_classes > 5 else (1, 1)
    batches, lines, epoch_lines = [], [], []
    for epoch in range(2):                  # the second epoch meets min_top1_err of the first
        for i, n in enumerate(sizes):
            # a permutation per row: distinct scores, torch.topk has no ties to break
            logits = np.stack([rng.permutation(num_classes) for _ in range(n)]).astype(np.float32) / np.float32(7)
            labels = rng.integers(0, num_classes, size=n)
            if i % 2 == 0:
                labels[0] = int(logits[0].argmax())
            extra = np.abs(f32(rng, 2)) + np.float32(0.5)
            preds, lab = torch.from_numpy(logits), torch.from_numpy(labels)
            correct = metrics.topks_correct(preds, lab, ks)
            top1, top5 = [(1.0 - x / preds.size(0)) * 100.0 for x in correct]
            again = metrics.topk_errors(preds, lab, ks)
            assert top1.item() == again[0].item() and top5.item() == again[1].item()
            meter.update_stats(top1.item(), top5.item(), n,
                               extra_metrices={"loss_ce": torch.tensor(extra[0]), "loss": torch.tensor(extra[1])})
            meter.log_iter_stats(epoch, i)
            lines.append(take(logged))
            batches.append({"epoch": epoch, "logits": enc(logits.tolist()), "labels": [int(v) for v in labels],
                            "extra": enc(extra.tolist()), "correct": [enc(float(c)) for c in correct]})
        meter.log_epoch_stats(epoch)
        epoch_lines.append(take(logged))
        meter.reset()
    return {"period": period, "num_classes": num_classes, "max_iter": len(sizes), "max_epoch": cfg.SOLVER.MAX_EPOCH,
            "extra_keys": ["loss_ce", "loss"], "batches": batches, "iter_lines": lines, "epoch_lines": epoch_lines}


def scalar_case(meters, rng):
    vals = f32(rng, 11).tolist()
    m = meters.ScalarMeter(4)
    out = []
    for v in vals:
        m.add_value(v)
        out.append([enc(m.get_win_median()), enc(m.get_win_avg()), enc(m.get_global_avg())])
    return {"window": 4, "values": enc(vals), "median_avg_global": out}


def main():
    meters, metrics, logged = load_reference()
    rng = np.random.default_rng(20240612)
    doc = {"scalar": scalar_case(meters, rng),
           "train": [train_case(meters, logged, p, rng) for p in (1, 3, 10)],
           "two_rank": two_rank_case(meters, logged, rng),
           "val": [val_case(meters, metrics, logged, c, rng) for c in (5, 174)]}
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
