"""The loops around the step: `train_epoch` and `eval_epoch` of the reference (tools/train_net.py:33-178, 181-368) for
single-label classification, without a host read per iteration.

What the reference does per iteration and this does per cfg.LOG_PERIOD: `.item()` on every entry of the loss dict
(train_net.py:153-167) and on the two top-k errors (train_net.py:325-335).  The numbers go through meters.TrainMeter /
meters.ValMeter, which keep them in device memory between periods; with a graph.GraphedTrainStep(meter=train_meter) the
push is part of the replayed step.

Not here: detection, Epic-Kitchens dict labels, multi-label mAP, `update_predictions` / TensorBoard, multigrid.
"""
import torch
import torch.distributed as dist

from . import losses, optim
from .graph import AccumulatedTrainStep, GraphedEvalStep, GraphedTrainStep
from .meters import log_json_stats


def _min_length(n):
    """du.all_gather_unaligned(len(loader)) -> min (train_net.py:73-74): ranks with loaders of different lengths stop
    together"""
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        got = [None] * dist.get_world_size()
        dist.all_gather_object(got, n)
        return min(got)
    return n


def _lr_value(lr):
    return lr["lr"] if isinstance(lr, dict) else lr


def accumulate_step(model, loss_funs, batches, optimizer, meter=None, lr=None):
    """The eager twin of graph.AccumulatedTrainStep: k recipe ranks (dp.virtual_roles) one after another on this GPU,
    ONE optimizer step.  `zero_grad` once, then per micro-step i the eager forward of batches[i] = (inputs, labels),
    loss_funs[i](preds, extra, labels) (a scalar, or a dict whose "loss" entry is differentiated) and its backward --
    every gradient producer ADDS into the flat buffer, nothing is zeroed in between and the weights do not move -- with
    a DataParallel wrapper the exchange from the last micro-step's backward only, then `optimizer.step()` with
    grad_scale / k: the step of the mean over the k (x world) recipe ranks.  meter: a TrainMeter(virtual_ranks=k).
    -> the k loss tensors."""
    k = len(batches)
    if k == 0 or len(loss_funs) != k:
        raise ValueError("accumulate_step: %d loss functions for %d batches" % (len(loss_funs), k))
    if not hasattr(optimizer, "grad_scale"):
        raise ValueError("accumulate_step needs an optimizer with a grad_scale (optim.FusedClipAdamW / GuardedClipAdamW), "
                         "got %s" % type(optimizer).__name__)
    core = model.module if hasattr(model, "module") else model
    if not core.training:
        raise RuntimeError("accumulate_step runs the training step: call model.train() first")
    if meter is not None and getattr(meter, "virtual_ranks", None) != k:
        raise ValueError("accumulate_step(meter=...) needs a TrainMeter(virtual_ranks=%d)" % k)
    optimizer.zero_grad()
    hook, out = core._grad_ready_hook, []
    try:
        for i, ((inputs, labels), loss_fun) in enumerate(zip(batches, loss_funs)):
            core._grad_ready_hook = hook if i == k - 1 else None      # the exchange rides on the last backward only
            preds, extra = model(inputs, {})
            got = loss_fun(preds, extra, labels)
            logged = got if isinstance(got, dict) else {"loss": got}
            logged["loss"].backward()
            out.append(logged["loss"].detach())
            if meter is not None:
                meter.push(logged, vrank=i)
    finally:
        core._grad_ready_hook = hook
    if meter is not None:
        world = getattr(model, "world_size", 1)
        meter.host_update(optimizer.param_groups[0]["lr"] if lr is None else lr,
                          sum(b[0][0].shape[0] for b in batches) * world)
    scale = optimizer.grad_scale
    optimizer.grad_scale = scale * (1.0 / k)
    try:
        optimizer.step()
    finally:
        optimizer.grad_scale = scale
    return out


def _train_epoch_accumulated(train_loader, step, optimizer, train_meter, cur_epoch, cfg):
    """train_epoch over an AccumulatedTrainStep: per iteration the loader yields k (inputs, labels, video_idx, meta) in
    virtual-rank order; a micro-step whose static labels are a dict (an image rank: the HAOG targets) takes `meta`"""
    if step.meter is not train_meter or step.optimizer is not optimizer:
        raise ValueError("train_epoch: the AccumulatedTrainStep must be built with the optimizer and meter= the ones "
                         "passed here (it ends with the optimizer's launches and pushes into the meter)")
    dev = step.x.device

    def to_dev(t):
        if isinstance(t, dict):
            return {k: to_dev(v) for k, v in t.items()}
        return t.to(dev, non_blocking=True) if torch.is_tensor(t) else t
    train_meter.iter_tic()
    data_size = len(train_loader)
    min_length = _min_length(data_size)
    for cur_iter, micro in enumerate(train_loader):
        if cur_iter >= min_length:
            break
        if len(micro) != len(step.micro_steps):
            raise ValueError("train_epoch: the loader yielded %d micro-batches, the step holds %d micro-steps"
                             % (len(micro), len(step.micro_steps)))
        batches = [([x.to(dev, non_blocking=True) for x in inputs],
                    to_dev(meta if isinstance(ms.static_labels, dict) else labels))
                   for ms, (inputs, labels, _vid_idx, meta) in zip(step.micro_steps, micro)]
        lr = _lr_value(optim.get_lr_at_epoch(cfg, cur_epoch + float(cur_iter) / data_size))
        optim.set_lr(optimizer, lr)
        train_meter.data_toc()
        step(batches)                                # (host half of update_stats included)
        train_meter.iter_toc()
        train_meter.log_iter_stats(cur_epoch, cur_iter)
        _log_tensor_stats(optimizer, cfg, cur_iter)
        _log_update_stats(optimizer, cfg, cur_iter)
        _log_activation_stats(step, cfg, cur_iter)
        _log_attention_stats(step, cfg, cur_iter)
        train_meter.iter_tic()
    stats = train_meter.log_epoch_stats(cur_epoch)
    train_meter.reset()
    return stats


def _train_epoch_fed(train_loader, step, optimizer, train_meter, cur_epoch, cfg, feeder):
    """train_epoch over a GraphedTrainStep and its feeder.ClipFeeder: the loader yields HOST batches
    (videos, records, labels, video_idx, meta[, randaug]); a step whose static labels are a dict (an image rank) takes
    `meta`.  One producer thread packs them into the feeder's pinned slots; per iteration `feeder.next()` (upload if not
    yet under way + one unpack launch into the step's static buffers), the replay, `feeder.pump()` -- batch n + 1
    uploads while step n runs."""
    from .feeder import Producer
    if not isinstance(step, GraphedTrainStep):
        raise ValueError("train_epoch(feeder=...) needs a GraphedTrainStep: the feeder writes its static buffers")
    if step.meter is not train_meter or step.optimizer is not optimizer:
        raise ValueError("train_epoch: the GraphedTrainStep must be built with optimizer= and meter= the ones passed "
                         "here (its replay ends with the optimizer's launches and holds the meter's push)")
    if feeder.target is not step.static_inputs[0]:
        raise ValueError("train_epoch: the feeder was built over another step's static input (ClipFeeder.for_step(step))")
    train_meter.iter_tic()
    data_size = len(train_loader)
    min_length = _min_length(data_size)
    from_meta = isinstance(step.static_labels, dict)

    def host_batches():
        for cur_iter, batch in enumerate(train_loader):
            if cur_iter >= min_length:
                break
            videos, records, labels, _vid_idx, meta = batch[:5]
            yield (videos, records, meta if from_meta else labels) + tuple(batch[5:6])
    producer = Producer(feeder, host_batches())
    producer.start()
    try:
        for cur_iter in range(min(min_length, data_size)):
            producer.wait_ready()
            inputs, labels = feeder.next()
            lr = _lr_value(optim.get_lr_at_epoch(cfg, cur_epoch + float(cur_iter) / data_size))
            optim.set_lr(optimizer, lr)
            train_meter.data_toc()
            step(inputs, labels)                     # (host half of update_stats included)
            feeder.pump()
            train_meter.iter_toc()
            train_meter.log_iter_stats(cur_epoch, cur_iter)
            _log_tensor_stats(optimizer, cfg, cur_iter)
            _log_update_stats(optimizer, cfg, cur_iter)
            _log_activation_stats(step, cfg, cur_iter)
            _log_attention_stats(step, cfg, cur_iter)
            train_meter.iter_tic()
    finally:
        producer.stop()
    stats = train_meter.log_epoch_stats(cur_epoch)
    train_meter.reset()
    return stats


def _log_monitor_stats(mon, cfg, cur_iter):
    """what the four functions below do with their monitor, or None: at the end of a cfg.LOG_PERIOD ONE read of its ring
    and, when that holds a row, one JSON line -> the line's dict or None"""
    if mon is None or (cur_iter + 1) % cfg.LOG_PERIOD != 0:
        return None
    stats = mon.log_stats(mon.read())
    if stats is not None:
        log_json_stats(stats)
    return stats


def _log_tensor_stats(optimizer, cfg, cur_iter):
    """once per cfg.LOG_PERIOD, with a monitor.TensorMonitor attached to the optimizer: ONE read of its ring and one JSON
    line {"_type": "train_tensor_stats", ...} -- norms per layer of the period's last recorded step, the culprits of its
    dropped steps.  Nothing without a monitor."""
    return _log_monitor_stats(getattr(optimizer, "monitor", None), cfg, cur_iter)


def _log_update_stats(optimizer, cfg, cur_iter):
    """once per cfg.LOG_PERIOD, with an updmon.UpdateMonitor attached to the optimizer: ONE read of its ring and one JSON
    line {"_type": "train_update_stats", ...} -- the step's and the weights' norm per layer of the period's last recorded
    step, the tensors most of whose elements did not move.  Nothing without a monitor."""
    return _log_monitor_stats(getattr(optimizer, "update_monitor", None), cfg, cur_iter)


def _log_activation_stats(step_or_model, cfg, cur_iter):
    """once per cfg.LOG_PERIOD, with an actmon.ActivationMonitor attached to the model (the step's, or the model itself):
    ONE read of its ring and one JSON line {"_type": "train_activation_stats", ...} -- the residual-stream RMS, the widest
    token's std and the largest attention log-sum-exp per block of the period's last pass, the origin of every pass with
    non-finite activations.  Nothing without a monitor."""
    core = getattr(step_or_model, "core", None) or getattr(step_or_model, "module", step_or_model)
    return _log_monitor_stats(getattr(getattr(core, "engine", None), "act_monitor", None), cfg, cur_iter)


def _log_attention_stats(step_or_model, cfg, cur_iter):
    """once per cfg.LOG_PERIOD, with an attnmon.AttentionMonitor attached to the model (the step's, or the model itself):
    ONE read of its ring and one JSON line {"_type": "train_attention_stats", ...} -- per block and query group the
    normalised entropy and the object-key mass of the period's last recorded pass, the head closest to collapse.
    Nothing without a monitor."""
    core = getattr(step_or_model, "core", None) or getattr(step_or_model, "module", step_or_model)
    return _log_monitor_stats(getattr(getattr(core, "engine", None), "attn_monitor", None), cfg, cur_iter)


def train_epoch(train_loader, step_or_model, optimizer, train_meter, cur_epoch, cfg, feeder=None):
    """tools/train_net.py:33-178.  step_or_model: a GraphedTrainStep built with `optimizer=` and `meter=train_meter`
    (the whole iteration is one replay; nothing here touches the device but the input copy) or the model itself (the
    eager step: forward, video_image_loss, backward, optimizer.step(), one meter push).  The loader yields
    (inputs, labels, video_idx, meta) like the reference's.  An AccumulatedTrainStep (k virtual ranks per iteration,
    graph.py) takes a loader that yields a list of k such tuples in virtual-rank order.
    feeder: a feeder.ClipFeeder over the GraphedTrainStep's static AugClips -- the loader then yields host batches
    (videos, records, labels, video_idx, meta[, randaug]) and uploads overlap the step (`_train_epoch_fed`).  None: the
    loop below."""
    if feeder is not None:
        return _train_epoch_fed(train_loader, step_or_model, optimizer, train_meter, cur_epoch, cfg, feeder)
    if isinstance(step_or_model, AccumulatedTrainStep):
        return _train_epoch_accumulated(train_loader, step_or_model, optimizer, train_meter, cur_epoch, cfg)
    graphed = isinstance(step_or_model, GraphedTrainStep)
    if graphed:
        if step_or_model.meter is not train_meter or step_or_model.optimizer is not optimizer:
            raise ValueError("train_epoch: the GraphedTrainStep must be built with optimizer= and meter= the ones passed "
                             "here (its replay ends with the optimizer's launches and holds the meter's push)")
        dev = step_or_model.x.device
    else:
        model = step_or_model
        model.train()
        dev = train_meter.device
        loss_fun = losses.get_loss_func(cfg)(reduction="mean")
        wloss = losses.get_lambdas_dict(cfg)
    train_meter.iter_tic()
    data_size = len(train_loader)
    min_length = _min_length(data_size)
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    for cur_iter, (inputs, labels, _vid_idx, meta) in enumerate(train_loader):
        if cur_iter >= min_length:
            break
        inputs = [x.to(dev, non_blocking=True) for x in inputs]
        labels = labels.to(dev, non_blocking=True)
        lr = _lr_value(optim.get_lr_at_epoch(cfg, cur_epoch + float(cur_iter) / data_size))
        optim.set_lr(optimizer, lr)
        train_meter.data_toc()
        if graphed:
            step_or_model(inputs, labels)            # (host half of update_stats included)
        else:
            meta = {k: v.to(dev, non_blocking=True) if torch.is_tensor(v) else v for k, v in (meta or {}).items()}
            preds, extra_preds = model(inputs, meta)
            loss_dict = loss_fun(preds, extra_preds, labels, meta)
            loss_dict["loss"] = sum(wloss[k] * loss_dict[k] for k in loss_dict)
            optimizer.zero_grad()
            loss_dict["loss"].backward()
            optimizer.step()
            train_meter.update_stats(lr, inputs[0].size(0) * world, dloss=loss_dict)
        train_meter.iter_toc()
        train_meter.log_iter_stats(cur_epoch, cur_iter)
        _log_tensor_stats(optimizer, cfg, cur_iter)
        _log_update_stats(optimizer, cfg, cur_iter)
        _log_activation_stats(step_or_model, cfg, cur_iter)
        _log_attention_stats(step_or_model, cfg, cur_iter)
        train_meter.iter_tic()
    stats = train_meter.log_epoch_stats(cur_epoch)
    train_meter.reset()
    return stats


def eval_extra_metrics(cfg, preds, extra_preds, labels, metadata):
    """slowfast/utils/meters.py:869-883: the validation losses as device tensors"""
    loss_fun = losses.get_loss_func(cfg, state="val")(reduction="mean")
    loss_fun.eval()
    loss_dict = loss_fun(preds, extra_preds, labels, metadata)
    wloss = losses.get_lambdas_dict(cfg)
    loss_dict["loss"] = sum(wloss[k] * loss_dict[k] for k in loss_dict if k in wloss)
    return loss_dict


def _eval_epoch_step(val_loader, step, val_meter, cur_epoch, cfg, feeder):
    """eval_epoch over a graph.GraphedEvalStep: an iteration is one replay (forward, frames pass, validation losses and
    the meter's push, its host half included), a short last batch the same body eagerly (`evaluate.run_eval_step`).
    `val_meter.data_toc()` is not called: the upload runs beside the previous replay (feeder) or lies with the loader, so
    the loop has no point at which the data of an iteration has arrived and its compute has not begun (the device
    meters' timers are no-ops and `time_diff` is wall time per read: meters.py)."""
    from .evaluate import run_eval_step
    if step.val_meter is not val_meter:
        raise ValueError("eval_epoch: the GraphedEvalStep must be built with val_meter= the meter passed here (its "
                         "replay holds the meter's push)")
    if bool(cfg.TRAIN.FORWARD_VIDEO_FRAMES) != bool(step.frames_pass) and step.x.shape[2] > 1:
        raise ValueError("eval_epoch: cfg.TRAIN.FORWARD_VIDEO_FRAMES is %s, the GraphedEvalStep was built with "
                         "frames_pass=%r" % (cfg.TRAIN.FORWARD_VIDEO_FRAMES, step.frames_pass))
    val_meter.iter_tic()

    def after(cur_iter):
        val_meter.iter_toc()
        val_meter.log_iter_stats(cur_epoch, cur_iter)
        val_meter.iter_tic()
    run_eval_step(val_loader, step, feeder, after)
    stats = val_meter.log_epoch_stats(cur_epoch)
    val_meter.reset()
    return stats


@torch.no_grad()
def eval_epoch(val_loader, model, val_meter, cur_epoch, cfg, feeder=None, ema=None):
    """tools/train_net.py:181-368, classification branch: per iteration one forward and one meter push (top-k hits and
    the extra losses), no host read between periods.
    ema: an ema.WeightEMA over this model -- the epoch runs inside `ema.average_weights()`, i.e. on the averaged weights
    (the raw ones are back, bit for bit, when it returns).  None: the loop below on the weights as they are.
    model: the model, or a graph.GraphedEvalStep built with `cfg=`, `val_meter=` this meter and the frames pass
    cfg.TRAIN.FORWARD_VIDEO_FRAMES asks for -- the loader then yields device-side (inputs, labels, ...); with `feeder` (a
    feeder.ClipFeeder over the step's static AugClips) it yields HOST batches (videos, records, labels, video_idx,
    meta) and uploads overlap the step."""
    if ema is not None:
        with ema.average_weights():
            return eval_epoch(val_loader, model, val_meter, cur_epoch, cfg, feeder=feeder)
    if isinstance(model, GraphedEvalStep):
        return _eval_epoch_step(val_loader, model, val_meter, cur_epoch, cfg, feeder)
    if feeder is not None:
        raise ValueError("eval_epoch(feeder=...) needs a GraphedEvalStep: the feeder writes its static buffers")
    model.eval()
    val_meter.iter_tic()
    dev = val_meter.device
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    for cur_iter, (inputs, labels, _, meta) in enumerate(val_loader):
        inputs = [x.to(dev, non_blocking=True) for x in inputs]
        labels = labels.to(dev, non_blocking=True)
        meta = {k: v.to(dev, non_blocking=True) if torch.is_tensor(v) else v for k, v in (meta or {}).items()}
        val_meter.data_toc()
        preds = model(inputs, meta)
        preds, extra_preds = preds if isinstance(preds, tuple) else (preds, None)
        if cfg.TRAIN.FORWARD_VIDEO_FRAMES and inputs[0].size(2) > 1:         # train_net.py:243-248
            _preds, _extra_preds = model([inputs[0].transpose(1, 2).flatten(0, 1).unsqueeze(2)], {})
            extra_preds["frames_output"] = {"preds": _preds, "extra_preds": _extra_preds}
        extra_metrics = eval_extra_metrics(cfg, preds, extra_preds, labels, meta)
        val_meter.iter_toc()
        val_meter.update_stats(preds, labels, inputs[0].size(0) * world, extra_metrices=extra_metrics)
        val_meter.log_iter_stats(cur_epoch, cur_iter)
        val_meter.iter_tic()
    stats = val_meter.log_epoch_stats(cur_epoch)
    val_meter.reset()
    return stats
