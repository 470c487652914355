"""Multi-view testing of SViT with the ensemble kept on the device.

Mirrors the reference's evaluation path for classification -- `perform_test`
(tools/test_net.py:25-170), `TestMeter` (slowfast/utils/meters.py:237-398), `topks_correct`
(slowfast/utils/metrics.py:9-50), the test-view table of the ssv2 dataset (slowfast/datasets/
ssv2.py:139-150,275-288) and `uniform_crop` (slowfast/datasets/transform.py:288-348) -- with three
changes that matter on an MI355X:

* the per-video accumulators live in HBM and a batch is folded by one launch
  (`svit_ensemble_update`): the eval loop has no device->host copy per iteration;
* data-parallel ranks keep private accumulators and merge them with ONE all-reduce at the end
  (`TestMeter.all_reduce`) instead of an all-gather of predictions, labels and indices per
  iteration (tools/test_net.py:147-150);
* in test mode the dataset's NUM_ENSEMBLE_VIEWS temporal views are identical frames (segment
  midpoints, ssv2.py:225-230): only the NUM_SPATIAL_CROPS unique views are computed and each is
  folded NUM_ENSEMBLE_VIEWS times (`unique_views`), 10x less forward work for the same scores.

On the uint8 route the views of a video are records over ONE uploaded copy of its frames (`test_views` ->
`augment.AugClips`), an iteration is one replay of a `graph.GraphedEvalStep` with the fold inside the graph, and host
batches arrive through `feeder.ClipFeeder` (`perform_test(..., feeder=)`, `run_eval_step`).  `head_eval_host` restates
the step's one new kernel, `svit_head_eval`, in NumPy.
"""
import math

import torch
import torch.distributed as dist

from . import hip
from .ops import ptr


class TestMeter:
    """slowfast/utils/meters.py:237-398 for single-label classification, device resident.
    Same constructor arguments, attributes (`video_preds`, `video_labels`, `clip_count`,
    `stats`) and methods the reference's callers use."""
    __test__ = False

    def __init__(self, num_videos, num_clips, num_cls, overall_iters, multi_label=False,
                 ensemble_method="sum", device=None):
        if multi_label:
            raise NotImplementedError("multi-label (mAP) ensembles are not part of the SViT path")
        if ensemble_method not in ("sum", "max"):
            raise NotImplementedError("Ensemble Method {} is not supported".format(ensemble_method))
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise hip.SvitHipError("TestMeter keeps its accumulators on the GPU; no CPU fallback")
        self.num_clips, self.overall_iters = num_clips, overall_iters
        self.multi_label, self.ensemble_method = multi_label, ensemble_method
        self.video_preds = torch.zeros((num_videos, num_cls), device=self.device)
        self.video_labels = torch.zeros((num_videos,), dtype=torch.int64, device=self.device)
        self.clip_count = torch.zeros((num_videos,), dtype=torch.int64, device=self.device)
        self.errors = torch.zeros(4, dtype=torch.int32, device=self.device)
        self.topk_accs, self.stats = [], {}

    def reset(self):
        self.clip_count.zero_()
        self.video_preds.zero_()
        self.video_labels.zero_()
        self.errors.zero_()

    def update_stats(self, preds, labels, clip_ids, metadata=None, extra_preds=None, repeat=1):
        """meters.py:303-336; everything stays on the device (no sync)."""
        preds = preds.detach().to(self.device, torch.float32).contiguous()
        labels = labels.to(self.device, torch.int64).contiguous()
        clip_ids = clip_ids.to(self.device, torch.int64).contiguous()
        n, c = preds.shape
        if c != self.video_preds.shape[1] or labels.numel() != n or clip_ids.numel() != n:
            raise ValueError("update_stats: preds %s labels %s clip_ids %s" % (
                tuple(preds.shape), tuple(labels.shape), tuple(clip_ids.shape)))
        hip.call("svit_ensemble_update", ptr(preds), ptr(labels), ptr(clip_ids), n, c,
                 self.num_clips, self.video_preds.shape[0],
                 0 if self.ensemble_method == "sum" else 1, int(repeat), ptr(self.video_preds),
                 ptr(self.video_labels), ptr(self.clip_count), ptr(self.errors))

    def all_reduce(self, group=None, force=False):
        """Merge the accumulators of data-parallel ranks (each saw a disjoint set of clips).  `force`: launch the four
        collectives on a one-rank group too (a rehearsal switch like DataParallel(force_collectives=True): the production
        backend's merge runs on the one GPU a test box has; SUM / MAX over one rank are the identity)."""
        if not (dist.is_available() and dist.is_initialized()):
            return
        if dist.get_world_size(group) == 1 and not force:
            return
        op = dist.ReduceOp.SUM if self.ensemble_method == "sum" else dist.ReduceOp.MAX
        dist.all_reduce(self.video_preds, op=op, group=group)
        dist.all_reduce(self.clip_count, op=dist.ReduceOp.SUM, group=group)
        dist.all_reduce(self.video_labels, op=dist.ReduceOp.MAX, group=group)
        dist.all_reduce(self.errors, op=dist.ReduceOp.SUM, group=group)

    def topks_correct(self, ks=(1, 5)):
        """metrics.topks_correct on the accumulators -> list of ints (the one host read)."""
        ks_t = torch.tensor(list(ks), dtype=torch.int32, device=self.device)
        counts = torch.zeros(len(ks), dtype=torch.int32, device=self.device)
        hip.call("svit_topk_correct", ptr(self.video_preds), ptr(self.video_labels),
                 self.video_preds.shape[0], self.video_preds.shape[1], ptr(ks_t), len(ks),
                 ptr(counts), ptr(self.errors))
        return [int(v) for v in counts.cpu()]

    def finalize_metrics(self, ks=(1, 5)):
        """meters.py:378-398."""
        correct = self.topks_correct(ks)
        err = [int(v) for v in self.errors.cpu()]
        if err[1]:
            raise AssertionError("%d clips disagree with their video's label" % err[1])
        if err[0] or err[2]:
            raise IndexError("clip ids / labels out of range: %s" % err[:3])
        self.stats = {"split": "test_final"}
        for k, c in zip(ks, correct):
            self.stats["top{}_acc".format(k)] = "{:.{prec}f}".format(
                c / self.video_preds.size(0) * 100.0, prec=2)
        return self.stats

    # timers / logging of the reference's meter: no-ops (host glue, SURVEY 2 "-")
    def iter_tic(self):
        pass

    def iter_toc(self):
        pass

    def data_toc(self):
        pass

    def log_iter_stats(self, cur_iter):
        pass


def unique_views(cfg):
    """-> (unique clips per video, repeat).  The ssv2 test set lists NUM_ENSEMBLE_VIEWS *
    NUM_SPATIAL_CROPS clips per video (ssv2.py:139-150) whose frames depend only on the spatial
    index `idx % NUM_SPATIAL_CROPS` (ssv2.py:275-288; temporal sampling = segment midpoints)."""
    return cfg.TEST.NUM_SPATIAL_CROPS, cfg.TEST.NUM_ENSEMBLE_VIEWS


def uniform_crop_offsets(height, width, size, spatial_idx):
    """transform.py:327-339."""
    if spatial_idx not in (0, 1, 2):
        raise AssertionError("spatial_idx must be 0, 1 or 2")
    y = int(math.ceil((height - size) / 2))
    x = int(math.ceil((width - size) / 2))
    if height > width:
        y = 0 if spatial_idx == 0 else (height - size if spatial_idx == 2 else y)
    else:
        x = 0 if spatial_idx == 0 else (width - size if spatial_idx == 2 else x)
    return y, x


def spatial_crops(video, size, num_crops=3):
    """video f32 [B,3,T,H,W] (short side already == size) -> [B*num_crops,3,T,size,size], the
    crops of one video adjacent and in spatial-index order (left/centre/right or top/mid/bottom)."""
    B, C, T, H, W = video.shape
    idx = [1] if num_crops == 1 else list(range(num_crops))
    out = torch.empty((B, len(idx), C, T, size, size), dtype=video.dtype, device=video.device)
    for j, s in enumerate(idx):
        y, x = uniform_crop_offsets(H, W, size, s)
        out[:, j] = video[:, :, :, y:y + size, x:x + size]
    return out.flatten(0, 1)


def test_views(sampler, sizes, first_video, num_crops):
    """The test-time views of a batch of videos as augmentation records over their shared uint8 frames (host only).
    sampler: `augment.build_sampler(cfg, "test")`; sizes: (h, w) of video v of the batch; first_video: the dataset index
    of video 0.  -> (records, clip_ids): video-major, for video v the records `sampler.draw(h, w, video=v,
    spatial_idx=s)` for s in range(num_crops), or the centre [1] when num_crops == 1 (ssv2.py:279-285; `spatial_crops`),
    and clip_ids int64 = (first_video + v) * num_crops + j."""
    idx = [1] if num_crops == 1 else list(range(num_crops))
    records, ids = [], []
    for v, (h, w) in enumerate(sizes):
        for j, s in enumerate(idx):
            records.append(sampler.draw(int(h), int(w), video=v, spatial_idx=s))
            ids.append((int(first_video) + v) * num_crops + j)
    return records, torch.tensor(ids, dtype=torch.int64)


test_views.__test__ = False          # (a library function: pytest must not collect it where a test imports it)


def head_eval_host(tokens, params, T, O, act, dtype=None):
    """NumPy restatement of svit_head_eval (include/svit_hip.h), float64 unless `dtype` says otherwise: the kernel's
    yardstick.  tokens [B,N,C] (row 0 = cls, the last T*O rows = objects); params = ((w, b) of the class projection, the
    box MLP, the objectness Linear, the contact MLP); act 0 softmax, 1 sigmoid.  -> (probabilities [B,n_cls], boxes
    [B,T,O,5], contact [B,T,2,5], obj_desc [B,T,O,C])."""
    import numpy as np
    dt = np.float64 if dtype is None else dtype

    def arr(t):
        return np.asarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t).astype(dt)

    def sigmoid(z):
        with np.errstate(over="ignore"):
            return (1 / (1 + np.exp(-z))).astype(dt)

    def softmax(z):
        e = np.exp(z - z.max(axis=-1, keepdims=True))
        return (e / e.sum(axis=-1, keepdims=True)).astype(dt)
    if act not in (0, 1):
        raise ValueError("act is 0 (softmax) or 1 (sigmoid)")
    x = arr(tokens)
    (wp, bp), (wb, bb), (we, be), (wc, bc) = [(arr(w), arr(b)) for w, b in params]
    B, N, C_ = x.shape
    if N < 1 + T * O:
        raise ValueError("N = %d rows cannot hold a cls row and %d x %d objects" % (N, T, O))
    z = x[:, 0] @ wp.T + bp
    probs = softmax(z) if act == 0 else sigmoid(z)
    xobj = x[:, N - T * O:].reshape(B, T, O, C_)
    boxes = np.concatenate((sigmoid(xobj @ we.T + be), sigmoid(xobj @ wb.T + bb)), axis=-1)
    contact = softmax(xobj[:, :, :2] @ wc.T + bc)
    return probs, boxes, contact, xobj


def _to_device(tree, dev):
    if isinstance(tree, dict):
        return {k: _to_device(v, dev) for k, v in tree.items()}
    return tree.to(dev, non_blocking=True) if torch.is_tensor(tree) else tree


def run_eval_step(loader, step, feeder=None, after=None):
    """What `perform_test` and `train.eval_epoch` share when they drive a graph.GraphedEvalStep: `step.refresh()` once,
    then every batch of `loader` through the replay (a full batch) or `step.eager` (a batch with fewer clips: the short
    last batch of an epoch), `after(cur_iter)` behind each.
    feeder None: the loader yields device-side (inputs, labels, ...) -- `labels` whatever the step's static labels hold.
    feeder (a feeder.ClipFeeder over the step's static AugClips): the loader yields HOST batches (videos, records,
    labels, ...); one feeder.Producer thread packs the full ones into the pinned slots and the loop is `next()` /
    replay / `pump()` as train._train_epoch_fed's.  A batch with fewer than V videos is not fed: it is reached in order,
    i.e. with every earlier batch consumed, and goes through `pack_videos(videos, Hs, Ws)`, a temporary AugClips with
    extents and `step.eager`."""
    import queue
    from .augment import AugClips, pack_videos
    from .graph import GraphedEvalStep
    if not isinstance(step, GraphedEvalStep):
        raise ValueError("expected a graph.GraphedEvalStep, got %s" % type(step).__name__)
    step.refresh()
    x = step.static_inputs[0]
    dev = x.device
    if feeder is None:
        for cur_iter, batch in enumerate(loader):
            inputs, labels = batch[0], batch[1]
            if inputs[0].shape[0] < x.shape[0]:
                step.eager(inputs, labels)
            else:
                step(inputs, labels)
            if after is not None:
                after(cur_iter)
        return
    from .feeder import Producer
    if feeder.target is not x:
        raise ValueError("the feeder was built over another step's static input (ClipFeeder.for_step(step))")
    if not isinstance(x, AugClips) or x.raw is not None:
        raise ValueError("a fed evaluation step runs over an AugClips without RandAugment")
    V, _, Hs, Ws, _ = x.frames.shape
    order = queue.Queue()           # per batch, in loader order: None (fed) or the short batch itself; _END last

    def host_batches():
        try:
            for batch in loader:
                videos, records, labels = batch[:3]
                if len(videos) == V:
                    order.put(None)
                    yield videos, records, labels
                else:
                    order.put((videos, records, labels))
        finally:                    # also when the loader raises: the loop ends and `producer.stop()` re-raises it
            order.put(_END)
    producer = Producer(feeder, host_batches())
    producer.start()
    try:
        cur_iter = 0
        while True:
            item = order.get()
            if item is _END:
                break
            if item is None:
                producer.wait_ready()       # (re-raises what `put` raised for this batch)
                inputs, labels = feeder.next()
                step(inputs, labels)
                feeder.pump()
            else:
                videos, records, labels = item
                frames, ext = pack_videos(list(videos), Hs, Ws)
                clips = AugClips(frames.to(dev, non_blocking=True), x.size, records, x.mean, x.std, lut_f32=x.lut_f32,
                                 extents=ext)
                step.eager([clips], _to_device(labels, dev))
            if after is not None:
                after(cur_iter)
            cur_iter += 1
    finally:
        producer.stop()


_END = object()


@torch.no_grad()
def perform_test(test_loader, model, test_meter, cfg, dedupe=True, force_collectives=False, feeder=None, ema=None):
    """tools/test_net.py:25-170, classification branch.  `test_loader` yields
    (inputs, labels, video_idx, meta) like the reference's loader; with `dedupe` it is expected to
    yield only the unique views (clip index = video * NUM_SPATIAL_CROPS + crop) and the meter is
    built with num_clips = NUM_SPATIAL_CROPS.
    model: the model, or a graph.GraphedEvalStep built with `test_meter=` this meter and `repeat=` the fold count used
    here -- the loader then yields device-side (inputs, {"labels", "clip_ids"}, ...) and an iteration is one replay
    (`run_eval_step`); with `feeder` (a feeder.ClipFeeder over the step) it yields HOST batches (videos, records,
    {"labels", "clip_ids"}, video_idx, meta) and uploads overlap the step.
    ema: an ema.WeightEMA over this model -- the test runs inside `ema.average_weights()`, on the averaged weights."""
    if ema is not None:
        with ema.average_weights():
            return perform_test(test_loader, model, test_meter, cfg, dedupe=dedupe, force_collectives=force_collectives,
                                feeder=feeder)
    repeat = unique_views(cfg)[1] if dedupe else 1
    ks = (1, 5) if cfg.MODEL.NUM_CLASSES > 5 else (1, 1)
    from .graph import GraphedEvalStep
    if isinstance(model, GraphedEvalStep):
        step = model
        if step.test_meter is not test_meter:
            raise ValueError("perform_test: the GraphedEvalStep must be built with test_meter= the meter passed here (its "
                             "replay holds the ensemble's fold)")
        if step.repeat != repeat:
            raise ValueError("perform_test folds every view %d times, the GraphedEvalStep was built with repeat=%d"
                             % (repeat, step.repeat))
        run_eval_step(test_loader, step, feeder)
        test_meter.all_reduce(force=force_collectives)
        test_meter.finalize_metrics(ks=ks)
        return test_meter
    if feeder is not None:
        raise ValueError("perform_test(feeder=...) needs a GraphedEvalStep: the feeder writes its static buffers")
    model.eval()
    for cur_iter, (inputs, labels, video_idx, meta) in enumerate(test_loader):
        preds = model(inputs, meta)
        if isinstance(preds, tuple):
            preds, _extra = preds
        test_meter.update_stats(preds, labels, video_idx, repeat=repeat)
    test_meter.all_reduce(force=force_collectives)
    test_meter.finalize_metrics(ks=ks)
    return test_meter
