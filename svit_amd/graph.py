"""HIP-graph replay of the SViT training step (forward + loss + backward).

The eager path (svit_amd/model.py) issues ~750 kernel launches per step from Python; most of
them run for 5-50 us on an MI355X, so the host is as busy as the GPU and every hiccup on the
host shows up as an idle GPU (profiles/README.md: ~13 % idle at B=8).  The launch schedule is
static for a fixed input shape, so it is captured ONCE into HIP graphs and replayed:

    step = GraphedTrainStep(model, loss_fun, inputs, labels)
    for inputs, labels in loader:
        loss, preds = step(inputs, labels)      # static tensors, overwritten by every replay
        optimizer.step()                        # eager (lr / bias correction are host scalars)

or, with the guarded optimizer (optim.GuardedClipAdamW keeps every scalar of its step in device memory), the whole step:

    step = GraphedTrainStep(model, loss_fun, inputs, labels, optimizer=optimizer)
    for inputs, labels in loader:
        set_lr(optimizer, lr)                   # reaches the replay: uploaded before the first segment
        loss, preds = step(inputs, labels)      # ends with the optimizer's launches; do NOT call optimizer.step()

What is inside the graph(s): bf16 weight refresh, grad-buffer memset, DropPath / dropout sampling
(torch's graph-safe Philox state), every backbone kernel, the head, `loss_fun`, the head's
autograd backward and the whole backbone backward.  Same arithmetic as the eager step
(tools/train_net.py:88-151 of the reference is the loop it replaces).

The capture is cut into segments wherever work leaves the main chain: (a) the engine's
grouped weight-gradient GEMM launches are replayed eagerly on a side stream next to the following segments -- inside one hipGraph the same fork/join ran slower
than serial on ROCm 7.2; (b) data parallel: after the segment that finalises a gradient bucket
the wrapper's `_on_ready` hook launches that bucket's all-reduce on RCCL's stream, overlapping
the next segment exactly like in the eager path (svit_amd/dp.py) -- no collective lives inside a
graph.

`GraphedEvalStep` (below) is the evaluation counterpart: one iteration of `train.eval_epoch` or `evaluate.perform_test` -- forward,
the eval-mode head as one launch, the frames pass, the meter's push or the ensemble's fold -- as ONE graph, a single chain on
one stream (nothing leaves the main chain without a backward).
"""
import gc
import warnings

import torch

from . import hip, ops


class GraphedTrainStep:
    def __init__(self, model, loss_fun, inputs, labels, warmup=2, frames_pass=False, mixup=None, optimizer=None,
                 meter=None, accumulate=False, input_grad=False):
        """model: SViT or its DataParallel wrapper (train mode); loss_fun(preds, extra, labels) ->
        scalar; inputs: the reference's `inputs` list ([video f32 [B,3,T,S,S]]); labels: any
        tensor (or tuple/dict of tensors) `loss_fun` takes -- copied into static buffers.  The static input may be an
        input.U8Clips or an augment.AugClips (uint8 frames + crop table / augmentation records, read by the im2col at
        replay time: `__call__` copies frames and table into the static ones).  Built with `extents=`, the static input
        is a padded buffer captured at its (Hs, Ws): `__call__` also copies the V x 8 bytes of the extents table and one
        capture serves batches of any mix of video sizes up to that buffer; a batch over a buffer of another shape is
        refused.
        frames_pass: also run the reference's no-grad single-frame forward of every clip
        (tools/train_net.py:105-110) inside the graph; its outputs reach `loss_fun` as
        extra["frames_output"] = {"preds", "extra_preds"} (the consistency-loss operand).  True: the fp32 route (the
        static input is the fp32 clip, permuted into B*T frames).  "u8": the static input is a U8Clips or an AugClips
        and the pass runs on input.FramesView(static input, fresh=True) -- the frames operand is assembled from the
        same uint8 frames and records (svit_im2col_patch_u8_aug_frames), no fp32 clip exists, the RandAugment chain of
        an AugClips runs once per step (ahead of the clip forward) and under `mixup` the view sees the step's record.
        mixup: a mixup.MixUp (cfg.MIXUP; `mixup.build_mixup(cfg)`) -- the step then OWNS a 32-byte mix record in
        device memory; the captured body starts with the clip kernel on the static input (or tags a U8Clips, whose
        im2col mixes) and `loss_fun` receives mixup.MixedLabels over the static labels (int64 [B]) instead of the
        labels.  Every kernel reads the record at replay time, so one capture serves mixup, CutMix and unmixed
        steps: `__call__` writes the step's record before the first segment.  The clip is mixed IN PLACE, as the
        reference mutates its input: a batch handed back in `static_inputs` is mixed where it lies and must be
        rewritten before the next replay.  The frames pass sees the mixed clip.  None: the same launches as ever.
        optimizer: an optim.GuardedClipAdamW over this model -- the captured body then ENDS with its launches (guard +
        AdamW, behind the last weight-gradient join; with data parallelism a last segment of its own, replayed after
        the final bucket's all-reduce has been waited for) and `__call__` uploads its host record before the first
        segment: the caller no longer calls `optimizer.step()`.  The warm-up runs of the body leave the tail out, so
        building the step moves no weight.  None: the same segments as ever.
        meter: a meters.TrainMeter on the step's device -- `loss_fun` may then return a dict (its "loss" entry is
        differentiated, as tools/train_net.py:124-125 adds it; the other entries are only logged; a scalar return logs
        {"loss": ...}) and the captured body holds the meter's push (one launch behind the loss: the row counter lives
        in device memory, every replay fills the next row of the ring).  `__call__` does the host half of
        `meter.update_stats` (lr -- the optimizer's, or the `lr` argument -- and mb_size = batch x ranks), so the loop
        only calls `meter.log_iter_stats`.  The warm-up runs only fix the meter's columns and the capture run executes
        nothing: the meter is empty after construction.  None: the same segments and launches as ever.
        accumulate: the step is a MICRO-step of an AccumulatedTrainStep (below) -- the captured body leaves out the bf16
        weight refresh and the gradient-buffer memset, so a replay ADDS this batch's gradients to what `flat.grad` holds;
        the owner issues both once per step, and the optimizer tail.  `optimizer=` and `meter=` are refused (the owner
        holds them).  False: the same segments and launches as ever.
        input_grad: the captured backward also computes d loss / d clip (one launch behind the stem's cast,
        svit_patch_embed_dgrad) into `step.input_grad`, a static f32 [B,3,T,S,S] every replay refills -- for an fp32
        clip, a U8Clips or an AugClips (in the coordinates of the S x S window; under `mixup`, with respect to the mixed
        clip).  Refused under a frozen cut.  False: the same segments and launches as ever.
        input_grad="only" (svit_amd/attribution.py): the step is an ATTRIBUTION pass, not a training step -- its captured
        body is forward, `loss_fun`, and the backward that computes the input gradient and NO parameter gradient
        (Engine.forward): ONE graph, no gradient memset and no bf16 weight refresh inside (the constructor refreshes once,
        `refresh()` after the weights moved, as GraphedEvalStep has it), no draw launch -- DropPath and the head's
        dropout are off whatever the cfg's rates.  A replay leaves flat.grad, every param.grad, weights, moments, meters,
        monitors and the draw counter as they are, and does not read the requires_grad flags: it works under a frozen
        cut.  `optimizer=`, `accumulate=True`, `frames_pass`, `meter=` and `mixup=` are refused."""
        self.accumulate = bool(accumulate)
        self.want_input_grad = bool(input_grad)
        self.only = isinstance(input_grad, str)
        if self.only:
            if input_grad != "only":
                raise hip.SvitHipError("input_grad is False, True or \"only\", got %r" % (input_grad,))
            for name, given in (("optimizer=", optimizer is not None), ("accumulate=True", accumulate),
                                ("frames_pass", frames_pass), ("meter=", meter is not None), ("mixup=", mixup is not None)):
                if given:
                    raise hip.SvitHipError("GraphedTrainStep(input_grad=\"only\") refuses %s: the step computes the "
                                           "input gradient of one clip forward and nothing else -- no parameter "
                                           "gradient exists for an optimizer, an accumulation or a meter to use" % name)
        self.input_grad = None
        if self.accumulate and (optimizer is not None or meter is not None):
            raise hip.SvitHipError("GraphedTrainStep(accumulate=True) is a micro-step: the optimizer tail and the meter "
                                   "belong to the AccumulatedTrainStep that replays it, pass optimizer= / meter= there")
        self.optimizer = optimizer
        self.meter = meter
        if meter is not None and torch.device(meter.device) != inputs[0].device:
            raise hip.SvitHipError("GraphedTrainStep(meter=...): the meter lives on %s, the step on %s"
                                   % (meter.device, inputs[0].device))
        if optimizer is not None:
            from .optim import GuardedClipAdamW
            if not isinstance(optimizer, GuardedClipAdamW):
                raise hip.SvitHipError(
                    "GraphedTrainStep(optimizer=...) takes an optim.GuardedClipAdamW, got %s: only its step reads every "
                    "scalar (lr, step counter, bias corrections) from device memory; any other optimizer's step holds "
                    "host scalars a replay would freeze -- call it eagerly after the replay" % type(optimizer).__name__)
            core = model.module if hasattr(model, "module") else model
            if optimizer.flat is not core.flat:
                raise hip.SvitHipError("GraphedTrainStep(optimizer=...): the optimizer was built over another model")
        self.frames_pass = frames_pass
        self.mixup = mixup
        self.wrapper = model
        self.core = model.module if hasattr(model, "module") else model
        if self.core.engine is None:
            raise hip.SvitHipError("GraphedTrainStep needs a finalized (on-GPU) SViT")
        if not self.core.training:
            raise RuntimeError("GraphedTrainStep captures the training step: call model.train() first")
        # frozen parameters (svit_amd/freeze.py): the flags are read HERE; the capture saves, back-propagates, exchanges and
        # steps for this cut only, so `__call__` refuses a replay once a flag has changed
        # (an input-gradient-only pass saves and back-propagates through every block whatever the flags say: not read)
        self.cut = 0 if self.only else self.core.frozen_cut()
        self._flag_params = list(self.core.parameters())
        self._flags = [p.requires_grad for p in self._flag_params]
        if self.want_input_grad and not self.only:
            _check_input_grad(self.cut)
        if optimizer is not None and optimizer.cut != self.cut:
            raise hip.SvitHipError("GraphedTrainStep(optimizer=...): the optimizer was built when the parameters' "
                                   "requires_grad flags froze everything below position %d, now they say %d -- rebuild "
                                   "the optimizer" % (optimizer.cut, self.cut))
        # the ema.WeightEMA attached to the optimizer NOW: its launch ends the captured tail (or none does)
        self._ema = optimizer.ema if optimizer is not None else None
        # ... and the monitor.TensorMonitor attached NOW: its two launches sit between the guard and the solver's
        self._monitor = optimizer.monitor if optimizer is not None else None
        # ... and the updmon.UpdateMonitor attached NOW: one launch in front of the solver's, two behind it
        self._update_monitor = getattr(optimizer, "update_monitor", None)
        # ... and the actmon.ActivationMonitor attached to the MODEL now: its two launches end the captured forward
        self._act_monitor = self.core.engine.act_monitor
        # ... and the attnmon.AttentionMonitor: two more behind those
        self._attn_monitor = getattr(self.core.engine, "attn_monitor", None)
        self.loss_fun = loss_fun
        self.dp = model if hasattr(model, "_on_ready") and (getattr(model, "world_size", 1) > 1 or
                                                           getattr(model, "force_collectives", False)) else None
        self.x = inputs[0].detach().clone().contiguous()
        from .augment import AugClips
        from .input import U8Clips
        if isinstance(frames_pass, str):
            if frames_pass != "u8":
                raise hip.SvitHipError("frames_pass is False, True or \"u8\", got %r" % (frames_pass,))
            if not isinstance(self.x, (U8Clips, AugClips)):
                raise hip.SvitHipError("frames_pass=\"u8\" reads the frames of a U8Clips or an AugClips; for the fp32 "
                                       "clip tensor pass frames_pass=True")
            self.x.lut_f32                    # (U8Clips: the fp32 table is built here, outside the capture)
        elif frames_pass and isinstance(self.x, AugClips):
            raise hip.SvitHipError("frames_pass=True is the fp32 route and does not take an AugClips: pass "
                                   "frames_pass=\"u8\" (or feed clips.render())")
        self.labels = _tree_map(lambda t: t.detach().clone(), labels)
        self.mix_record = self.loss_labels = None
        if mixup is not None:
            from .mixup import NO_MIX
            if not torch.is_tensor(self.labels) or self.labels.dtype != torch.int64 or self.labels.dim() != 1:
                raise hip.SvitHipError("GraphedTrainStep(mixup=...) needs int64 [B] labels")
            if self.x.shape[0] < 2:
                raise hip.SvitHipError("mixup needs a batch of at least 2 clips")
            # "no mix" while the body runs for warm-up and capture: those launches leave the static input as it is
            self.mix_record = torch.from_numpy(NO_MIX.pack()).to(self.x.device)
            self.loss_labels = mixup.labels(self.labels, self.mix_record)
            self._mix_slots = torch.empty((16, 8), dtype=torch.int32).pin_memory()
            self._mix_events, self._mix_next = [None] * 16, 0
            if not torch.is_tensor(self.x):
                self.x.lut_f32                # (U8Clips / AugClips: the fp32 table is built here, outside the capture)
                self.x.mix = self.mix_record
        self.segments = []          # replay items: ("graph", CUDAGraph) | ("side", fn) | ("join", None) | ("ready", ranks)
        self.loss = self.preds = self.extra = None
        self._keepalive = None
        self._capture(warmup)

    # ------------------------------------------------------------------------------------------
    def _loss(self, preds, extra, labels, tail):
        """loss_fun -> the scalar to differentiate; with a meter, the push of what it returned (warm-up runs: the column
        names only)"""
        out = self.loss_fun(preds, extra, labels)
        if isinstance(out, dict):
            if "loss" not in out:
                raise hip.SvitHipError("loss_fun returned a dict without a \"loss\" entry: %s" % sorted(out))
            loss, logged = out["loss"], out
        else:
            loss, logged = out, {"loss": out}
        if self.meter is not None:
            (self.meter.push if tail else self.meter.bind)(logged)
        self.loss_dict = {k: v.detach() for k, v in logged.items() if torch.is_tensor(v)}
        return loss

    def refresh(self):
        """input_grad="only": the bf16 copies of the weights, eagerly on the current stream -- call it after the weights
        moved (the captured body holds no refresh)"""
        with torch.no_grad():
            self.core.engine.refresh_weights()

    def _body_only(self):
        """the body of an input_grad="only" step: forward, loss_fun, the backward without parameter gradients"""
        core = self.core
        eng, x = core.engine, self.x
        Tx = x.shape[2] if x.dim() == 5 else 1
        with torch.no_grad():
            y, st = eng.forward(x, None, save=True, cut=0, input_grad="only")
        yt = y.detach().requires_grad_(True)
        with torch.enable_grad():
            if core.fused_head:
                preds, extra = core.head_train(yt, Tx, lean=True)
            else:
                from .model import _lean_head
                n_obj = Tx * core.O
                preds, extra = _lean_head(core.head, torch.cat((yt[:, :1], yt[:, -n_obj:]), dim=1), Tx, None)
            loss = self._loss(preds, extra, self.labels, False)
        dy, = torch.autograd.grad(loss, [yt])
        with torch.no_grad():
            eng.backward(st, dy)
        return (loss.detach(), preds.detach(),
                {k: v.detach() for k, v in extra.items() if torch.is_tensor(v)}, (st, yt, dy))

    def _body(self, boundary, tail=False):
        if self.only:
            return self._body_only()
        core = self.core
        eng, flat = core.engine, core.flat
        x = self.x
        Tx = x.shape[2] if x.dim() == 5 else 1
        labels = self.labels
        if self.mixup is not None:
            labels = self.loss_labels
            if torch.is_tensor(x):
                ops.mixup_clips(x, self.mix_record)      # in place; a U8Clips / AugClips is mixed by its im2col instead
        if not self.accumulate:         # (a micro-step: once per step, by the AccumulatedTrainStep)
            eng.refresh_weights()
            flat.grad.zero_()
        ds = core.sample_drop_scales(x.shape[0], x.device, Tx=Tx)      # (+ the head's dropout factors: one launch)
        head_keep, core._head_keep = core._head_keep, None
        with torch.no_grad():
            # (the head alone trainable: nothing is kept, and backward() below only reports the ranks)
            y, st = eng.forward(x, ds, save=self.cut <= len(core.plan.blocks) + 1, cut=self.cut,
                                input_grad=self.want_input_grad)
        n_obj = Tx * core.O
        frames_out = None
        if self.frames_pass and Tx > 1:
            with torch.no_grad():       # B*T single frames through the same kernels (T' = 1)
                if self.frames_pass == "u8":            # (the clip forward above has run the RandAugment chain)
                    from .input import FramesView
                    xf = FramesView(x, fresh=True)
                else:
                    xf = x.transpose(1, 2).flatten(0, 1).unsqueeze(2)
                fy, _ = eng.forward(xf, core.sample_drop_scales(xf.shape[0], x.device), save=False)
                ffeat = torch.cat((fy[:, :1], fy[:, -core.O:]), dim=1)
                fp, fe = core.head(ffeat, T=1)
                frames_out = {"preds": fp, "extra_preds": fe}
        if core.fused_head:
            # the head as one launch each way (csrc/head.hip): its backward writes the head's parameter
            # gradients straight into the flat buffer's views and returns d(tokens) whole -- no AccumulateGrad
            # node of a real parameter is involved (those may be pinned to another stream by an earlier eager
            # step, which a stream capture cannot follow), no slice / cat plumbing either
            yt = y.detach().requires_grad_(True)
            with torch.enable_grad():
                preds, extra = core.head_train(yt, Tx, dropout_keep=head_keep)
                if frames_out is not None:
                    extra = dict(extra)
                    extra["frames_output"] = frames_out
                loss = self._loss(preds, extra, labels, tail)
            dy, = torch.autograd.grad(loss, [yt])
            feat = yt
        else:
            feat = torch.cat((y[:, :1], y[:, -n_obj:]), dim=1).requires_grad_(True)
            # the head runs on fresh leaf aliases of its parameters and explicit autograd.grad instead
            # of loss.backward(): AccumulateGrad nodes of the real parameters may be pinned to another
            # stream by an earlier eager step, which a stream capture cannot follow
            named = list(core.head.named_parameters())
            alias = {n: p.detach().requires_grad_(True) for n, p in named}
            with torch.enable_grad():
                preds, extra = torch.func.functional_call(core.head, alias, (feat,), {"T": Tx})
                if frames_out is not None:
                    extra = dict(extra)
                    extra["frames_output"] = frames_out
                loss = self._loss(preds, extra, labels, tail)
            grads = torch.autograd.grad(loss, [feat] + [alias[n] for n, _ in named], allow_unused=True)
            with torch.no_grad():
                for (n, p), g in zip(named, grads[1:]):
                    if g is not None:
                        p.grad.add_(g)
                dfeat = grads[0]
                dy = torch.zeros_like(y)
                dy[:, :1] = dfeat[:, :1]
                dy[:, -n_obj:] = dfeat[:, 1:]
        with torch.no_grad():
            eng.backward(st, dy, on_ready=boundary,
                         ready_ranks=self.dp.launch_ranks() if self.dp is not None else None)
            if tail and self.optimizer is not None:
                # every gradient is final here: backward() ends behind its last flush and join, and with data parallelism
                # the final rank's boundary has just cut the capture, so these launches open a segment of their own
                self.optimizer.enqueue()
        return (loss.detach(), preds.detach(),
                {k: v.detach() for k, v in extra.items() if torch.is_tensor(v)}, (st, feat, dy))

    def _capture(self, warmup):
        core = self.core
        eng = core.engine
        if not self.only:
            core._attach_grads()                  # .grad views of the flat buffer, host side only
        if self.accumulate or self.only:          # (what the owner's prologue does in front of every step)
            self.refresh()
        dev = self.x.device
        cap = torch.cuda.Stream(device=dev)
        cap.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(cap):
            for _ in range(max(1, warmup)):       # lazy tables / library workspaces materialise here
                self._body(None)
        cap.synchronize()
        gc.collect()
        torch.cuda.empty_cache()
        pool = torch.cuda.graph_pool_handle()
        cuts = self.dp.launch_ranks() if self.dp is not None else set()
        # "thread_local": the process group's watchdog thread may query events while we capture
        mode = "thread_local"
        state = {"g": None}

        def begin():
            state["g"] = torch.cuda.CUDAGraph()
            state["g"].capture_begin(pool=pool, capture_error_mode=mode)

        def end():
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                state["g"].capture_end()
            if not any("Graph is empty" in str(x.message) for x in w):
                self.segments.append(("graph", state["g"]))

        def cut(item):
            """close the running capture, queue `item` for replay, open the next capture"""
            end()
            self.segments.append(item)
            begin()

        seen = []

        def boundary(rank):
            seen.append(rank)
            if rank in cuts:
                cut(("ready", list(seen)))
                seen.clear()

        eng._capture_fork = lambda fn: cut(("side", fn))
        eng._capture_join = lambda: cut(("join", None))
        try:
            with torch.cuda.stream(cap):
                begin()
                try:
                    self.loss, self.preds, self.extra, self._keepalive = self._body(
                        boundary if self.dp is not None else None, tail=True)
                finally:
                    end()
        finally:
            eng._capture_fork = eng._capture_join = None
        if self.want_input_grad:        # allocated inside the capture: the graph's pool keeps it, every replay refills it
            self.input_grad = self._keepalive[0]["dvideo"]
        torch.cuda.current_stream(dev).wait_stream(cap)
        torch.cuda.synchronize(dev)
        self._side = torch.cuda.Stream(device=dev)

    # ------------------------------------------------------------------------------------------
    def check_flags(self):
        """refuse a replay after a `requires_grad` flag has changed: the capture holds the old cut's launches"""
        if self.only:       # (reads no flag and pushes no monitor)
            return
        if [p.requires_grad for p in self._flag_params] != self._flags:
            raise hip.SvitHipError("a parameter's requires_grad changed after this GraphedTrainStep was captured (it "
                                   "froze everything below position %d): rebuild the optimizer and the step" % self.cut)
        _check_act_monitor(self.core, self._act_monitor, "GraphedTrainStep")
        _check_attn_monitor(self.core, self._attn_monitor, "GraphedTrainStep")
        if self.optimizer is not None:
            _check_ema(self.optimizer, self._ema, "GraphedTrainStep")
            _check_monitor(self.optimizer, self._monitor, "GraphedTrainStep")
            _check_update_monitor(self.optimizer, self._update_monitor, "GraphedTrainStep")

    def check_batch(self, inputs):
        """refuse a batch the capture does not fit (before anything is enqueued)"""
        self.check_flags()
        x = inputs[0]
        if x.shape != self.x.shape:
            raise hip.SvitHipError("GraphedTrainStep was captured for input %s, got %s"
                                   % (tuple(self.x.shape), tuple(x.shape)))
        if not torch.is_tensor(x):
            # uint8 route: the kernels were captured with the static buffer's (Hs, Ws) as launch arguments; videos of
            # other sizes travel inside a buffer of that shape with their extents (augment.pack_videos(..., Hs, Ws))
            if not hasattr(x, "frames") or x.frames.shape != self.x.frames.shape:
                raise hip.SvitHipError("GraphedTrainStep was captured for a frame buffer %s, got %s: pad the batch to "
                                       "the captured size and pass the videos' extents"
                                       % (tuple(self.x.frames.shape), tuple(getattr(x, "frames", x).shape)))

    def __call__(self, inputs, labels, mix=None, lr=None, exchange=True):
        """mix: this step's mixup.MixRecord (mixup steps only; drawn from np.random when None, as the reference's
        MixUp call would).  lr: what the meter logs for this step when the step holds no optimizer.  exchange: False
        skips the data-parallel launch points of this replay (an AccumulatedTrainStep's micro-steps but the last)."""
        self.check_batch(inputs)
        x = inputs[0]
        if x.data_ptr() != self.x.data_ptr():
            self.x.copy_(x, non_blocking=True)
        _tree_copy(self.labels, labels)
        if self.mixup is not None:
            rec = self.mixup.draw(self.x.shape) if mix is None else mix
            # 32 bytes, in stream order before the first segment, without stalling the host: a ring of pinned slots,
            # each guarded by the event of the copy that last read it
            i = self._mix_next
            self._mix_next = (i + 1) % len(self._mix_events)
            if self._mix_events[i] is not None:
                self._mix_events[i].synchronize()
            self._mix_slots[i].copy_(torch.from_numpy(rec.pack()))
            self.mix_record.copy_(self._mix_slots[i], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.x.device))
            self._mix_events[i] = ev
        elif mix is not None:
            raise hip.SvitHipError("a mix record was passed to a GraphedTrainStep built without mixup")
        if self.optimizer is not None:
            self.optimizer.upload()
        if self.meter is not None:
            if lr is None and self.optimizer is not None:
                lr = self.optimizer.param_groups[0]["lr"]
            self.meter.host_update(lr, self.x.shape[0] * getattr(self.wrapper, "world_size", 1))
        main = torch.cuda.current_stream(self.x.device)
        for kind, val in self.segments:
            if kind == "graph":
                val.replay()
            elif kind == "side":        # parameter-gradient work next to the following segments
                self._side.wait_stream(main)
                with torch.cuda.stream(self._side):
                    val()
            elif kind == "join":
                main.wait_stream(self._side)
            elif exchange:              # "ready": this bucket's gradients are final -> all-reduce
                for r in val:
                    self.dp._on_ready(r)
        return self.loss, (self.preds, self.extra)

    @property
    def static_inputs(self):
        """the buffers the captured step reads: a loader that makes them the TARGET of its host-to-device copy and
        passes them back to __call__ saves the device-to-device copy of every step (77 MB at B = 8, 16x224^2 fp32)"""
        return [self.x]

    @property
    def static_labels(self):
        return self.labels

    @property
    def n_graphs(self):
        return sum(1 for k, _ in self.segments if k == "graph")


class AccumulatedTrainStep:
    """k recipe ranks ("virtual ranks", dp.virtual_roles) on one GPU: k captured micro-steps add their gradients into
    the one flat buffer, then ONE exchange and ONE optimizer step -- the cfg.NUM_GPUS-rank step of the recipe on any
    divisor of that many GPUs.

        video = GraphedTrainStep(model, video_loss, [clips], labels, accumulate=True)
        image = GraphedTrainStep(model, image_loss, [stills], meta, accumulate=True)
        step = AccumulatedTrainStep(model, [video] * 7 + [image], optimizer, meter=train_meter)
        losses = step(batches)            # [(inputs, labels)] * 8 in virtual-rank order

    Per call: the bf16 weight refresh and the gradient-buffer memset once; every micro-step's replay (its own batch,
    its own DropPath / dropout draws -- the draw counter advances per replay -- its own mix record, frames pass and
    RandAugment chain); with a DataParallel wrapper the bucketed all-reduce from the launch points of the LAST
    micro-step only (overlapping its backward; the earlier ones skip theirs), which leaves the mean over the real
    ranks; then the guarded tail with grad_scale / k: norm, clip coefficient and update are those of the mean over all
    k x world recipe ranks, and one non-finite micro-step drops the whole step.  Prologue and tail are eager launches
    (about ten per step, plus a 4-byte loss copy per micro-step), the hot path is the micro-steps' graphs.

    micro_steps: k GraphedTrainStep(accumulate=True) over `model`; entries of equal shape and role may be the SAME
    object (one capture replayed for several virtual ranks).  meter: a meters.TrainMeter(virtual_ranks=k); each
    micro-step's loss dict is pushed into its own ring behind its replay (one launch), the host half (lr, mb_size =
    sum of the micro-batches x real ranks) once per step."""

    def __init__(self, model, micro_steps, optimizer, meter=None):
        from .optim import GuardedClipAdamW
        self.wrapper = model
        self.core = core = model.module if hasattr(model, "module") else model
        self.micro_steps = list(micro_steps)
        self.k = k = len(self.micro_steps)
        if k == 0:
            raise hip.SvitHipError("AccumulatedTrainStep needs at least one micro-step")
        if core.engine is None:
            raise hip.SvitHipError("AccumulatedTrainStep needs a finalized (on-GPU) SViT")
        if not core.training:
            raise RuntimeError("AccumulatedTrainStep runs the training step: call model.train() first")
        if not isinstance(optimizer, GuardedClipAdamW):
            raise hip.SvitHipError(
                "AccumulatedTrainStep takes an optim.GuardedClipAdamW, got %s: its tail reads grad_scale = 1/k and every "
                "other scalar from device memory and drops a step with a non-finite micro-step on the device"
                % type(optimizer).__name__)
        if optimizer.flat is not core.flat:
            raise hip.SvitHipError("AccumulatedTrainStep: the optimizer was built over another model")
        self.dp = model if hasattr(model, "_on_ready") and (getattr(model, "world_size", 1) > 1 or
                                                           getattr(model, "force_collectives", False)) else None
        for i, ms in enumerate(self.micro_steps):
            if not isinstance(ms, GraphedTrainStep):
                raise hip.SvitHipError("micro-step %d is a %s, not a GraphedTrainStep" % (i, type(ms).__name__))
            if ms.core is not core:
                raise hip.SvitHipError("micro-step %d was built over another model: its gradients land in another flat "
                                       "buffer" % i)
            if ms.optimizer is not None:
                raise hip.SvitHipError("micro-step %d was built with its own optimizer=: it would step the weights "
                                       "between the micro-steps" % i)
            if not ms.accumulate:
                raise hip.SvitHipError("micro-step %d was built without accumulate=True: its replay zeroes the gradient "
                                       "buffer" % i)
            if ms.dp is not self.dp:
                raise hip.SvitHipError("micro-step %d and the AccumulatedTrainStep disagree about the data-parallel "
                                       "wrapper: build both over the same DataParallel (or both over the bare model)" % i)
            if ms.cut != optimizer.cut:
                raise hip.SvitHipError("micro-step %d was captured with everything below position %d frozen, the "
                                       "optimizer with %d: rebuild them over the same requires_grad flags"
                                       % (i, ms.cut, optimizer.cut))
        self.optimizer = optimizer
        self._ema = optimizer.ema           # (the tail is eager, but a step is built for one recipe: as the freeze flags)
        self._monitor = optimizer.monitor
        self._update_monitor = getattr(optimizer, "update_monitor", None)
        self._act_monitor = core.engine.act_monitor
        self._attn_monitor = getattr(core.engine, "attn_monitor", None)
        self.meter = meter
        if meter is not None:
            if getattr(meter, "virtual_ranks", None) != k:
                raise hip.SvitHipError("AccumulatedTrainStep(meter=...) needs a TrainMeter(virtual_ranks=%d): video and "
                                       "image micro-steps log different keys, each into its own ring" % k)
            if torch.device(meter.device) != self.micro_steps[0].x.device:
                raise hip.SvitHipError("AccumulatedTrainStep(meter=...): the meter lives on %s, the step on %s"
                                       % (meter.device, self.micro_steps[0].x.device))
        # micro-steps that share a capture share its static loss tensor: every replay's loss is copied out (4 bytes)
        self._loss_buf = torch.zeros(k, dtype=torch.float32, device=self.micro_steps[0].x.device)
        self.losses = list(self._loss_buf.unbind(0))

    def _check(self, batches):
        if not self.core.training:
            raise RuntimeError("AccumulatedTrainStep runs the training step: call model.train() first")
        if len(batches) != self.k:
            raise hip.SvitHipError("AccumulatedTrainStep holds %d micro-steps, got %d batches" % (self.k, len(batches)))
        _check_act_monitor(self.core, self._act_monitor, "AccumulatedTrainStep")
        _check_attn_monitor(self.core, self._attn_monitor, "AccumulatedTrainStep")
        self.micro_steps[0].check_flags()       # (every micro-step holds the optimizer's cut)
        _check_ema(self.optimizer, self._ema, "AccumulatedTrainStep")
        _check_monitor(self.optimizer, self._monitor, "AccumulatedTrainStep")
        _check_update_monitor(self.optimizer, self._update_monitor, "AccumulatedTrainStep")
        for i, (ms, b) in enumerate(zip(self.micro_steps, batches)):
            if _is_feeder(b):
                if b.target is not ms.x:
                    raise hip.SvitHipError("micro-step %d: the feeder was built over another step's static input" % i)
                continue
            try:
                ms.check_batch(b[0])
            except hip.SvitHipError as e:
                raise hip.SvitHipError("micro-step %d: %s" % (i, e)) from None

    def __call__(self, batches, mixes=None, lr=None):
        """batches: k (inputs, labels) in virtual-rank order -- an entry may instead be the feeder.ClipFeeder of its
        micro-step's capture (one feeder may stand at several entries): its `next()` is called immediately before that
        micro-step's replay and `pump()` once behind the last one; mixes: per micro-step its mixup.MixRecord or None (mixup
        micro-steps draw their own when None).  -> the k loss tensors (0-d views of one static buffer, overwritten by the
        next call)."""
        self._check(batches)            # (nothing is enqueued for a step that is refused)
        core, opt, k = self.core, self.optimizer, self.k
        with torch.no_grad():
            core.engine.refresh_weights()
            core.flat.grad.zero_()
        if self.meter is not None:
            world = getattr(self.wrapper, "world_size", 1)
            self.meter.host_update(opt.param_groups[0]["lr"] if lr is None else lr,
                                   sum(ms.x.shape[0] for ms in self.micro_steps) * world)
        for i, (ms, b) in enumerate(zip(self.micro_steps, batches)):
            # a feeder: micro-steps that share a capture share its static buffer, so the batch is unpacked into it
            # immediately before its own replay
            inputs, labels = b.next() if _is_feeder(b) else b
            ms(inputs, labels, mix=mixes[i] if mixes is not None else None, exchange=i == k - 1)
            self.losses[i].copy_(ms.loss)
            if self.meter is not None:
                self.meter.push(ms.loss_dict, vrank=i)
        fed = []
        for b in batches:                # the next step's uploads run beside this step's tail
            if _is_feeder(b) and not any(b is f for f in fed):
                fed.append(b)
                b.pump()
        # the tail of the mean over the k virtual ranks: this step's record carries grad_scale / k, the optimizer keeps its own
        scale = opt.grad_scale
        opt.grad_scale = scale * (1.0 / k)
        try:
            opt.upload()
        finally:
            opt.grad_scale = scale
        with torch.no_grad():
            opt.enqueue()
        return self.losses

    step = __call__

    @property
    def x(self):
        return self.micro_steps[0].x


class GraphedEvalStep:
    """HIP-graph replay of one evaluation iteration (tools/train_net.py:181-368 per `TRAIN.EVAL_PERIOD`, tools/test_net.py:
    25-170 at the end): backbone forward, the eval-mode head as one launch (`SViT.head_eval`, csrc/head_eval.hip), the
    frames pass, the validation losses + meter push or the test ensemble's fold -- ONE graph, a single chain of kernel
    nodes on one stream.  The bf16 weight refresh is NOT in the captured body: weights do not move during an
    evaluation, so `refresh()` issues it eagerly -- the constructor calls it once, `train.eval_epoch` and
    `evaluate.perform_test` once before their first batch, and a caller that replays the step by hand after the weights
    changed calls it itself.

        model.eval()
        step = GraphedEvalStep(model, [clips], {"labels": y, "clip_ids": ids}, test_meter=meter, repeat=10)
        feeder = ClipFeeder.for_step(step)                  # static_inputs / static_labels: GraphedTrainStep's contract
        evaluate.perform_test(loader, step, meter, cfg, feeder=feeder)

    model: an SViT or its DataParallel wrapper in eval mode (a model in training mode is refused).  inputs: [AugClips],
    [U8Clips] or [fp32 tensor], the shapes a replay will see.  labels: int64 [B], or the tree {"labels": int64 [B],
    "clip_ids": int64 [B]} of a test batch; copied into static buffers (`static_labels`).
    frames_pass: "u8" (U8Clips / AugClips: `input.FramesView(x, fresh=True)`) or True (fp32) -- with more than one frame
    the single-frame forward of tools/train_net.py:243-248 runs too and arrives as extra["frames_output"].
    val_meter (needs cfg): `train.eval_extra_metrics` and the meter's push are part of the body and `__call__` / `eager`
    do the host half, so the loop only calls `log_iter_stats`.  test_meter: `update_stats(preds, labels, clip_ids,
    repeat=repeat)` is part of the body; the warm-up runs leave it out, so the meter is empty after construction.
    The step draws nothing (`sample_drop_scales` is never called) and writes neither weights, gradients nor optimizer
    state."""

    def __init__(self, model, inputs, labels, *, cfg=None, frames_pass=False, val_meter=None, test_meter=None, repeat=1,
                 warmup=2):
        from .augment import AugClips
        from .input import U8Clips
        self.wrapper = model
        self.core = core = model.module if hasattr(model, "module") else model
        if core.engine is None:
            raise hip.SvitHipError("GraphedEvalStep needs a finalized (on-GPU) SViT")
        if core.training:
            raise hip.SvitHipError("GraphedEvalStep captures the evaluation step: call model.eval() first (the training "
                                   "step is graph.GraphedTrainStep)")
        try:        # an unsupported pattern of requires_grad flags is refused here as well; evaluation itself ignores the flags
            core.frozen_cut()
        except ValueError:
            pass    # (nothing trainable: an evaluation needs no optimizer)
        if val_meter is not None and cfg is None:
            raise hip.SvitHipError("GraphedEvalStep(val_meter=...) needs cfg=: the validation losses are built from it")
        dev = inputs[0].device
        for name, m in (("val_meter", val_meter), ("test_meter", test_meter)):
            if m is not None and torch.device(m.device) != dev:
                raise hip.SvitHipError("GraphedEvalStep(%s=...): the meter lives on %s, the step on %s" % (name, m.device, dev))
        self.cfg, self.val_meter, self.test_meter, self.repeat = cfg, val_meter, test_meter, int(repeat)
        self.frames_pass = frames_pass
        self.x = inputs[0].detach().clone().contiguous()
        if isinstance(frames_pass, str):
            if frames_pass != "u8":
                raise hip.SvitHipError("frames_pass is False, True or \"u8\", got %r" % (frames_pass,))
            if not isinstance(self.x, (U8Clips, AugClips)):
                raise hip.SvitHipError("frames_pass=\"u8\" reads the frames of a U8Clips or an AugClips; for the fp32 "
                                       "clip tensor pass frames_pass=True")
        elif frames_pass and isinstance(self.x, AugClips):
            raise hip.SvitHipError("frames_pass=True is the fp32 route and does not take an AugClips: pass "
                                   "frames_pass=\"u8\" (or feed clips.render())")
        if not torch.is_tensor(self.x):
            self.x.lut_f32                    # (U8Clips: the fp32 table is built here, outside the capture)
        self.labels = _tree_map(lambda t: t.detach().clone().contiguous(), labels)
        self._split(self.labels)              # (refuses a tree the meters cannot be fed from)
        self.graph = self.preds = self.extra = None
        self.refresh()
        self._capture(warmup)

    # ------------------------------------------------------------------------------------------
    def _split(self, labels):
        """-> (labels int64 [B], clip_ids or None) of a label tree"""
        if isinstance(labels, dict):
            if "labels" not in labels:
                raise hip.SvitHipError("the label tree of an evaluation step holds \"labels\" (and \"clip_ids\" for the "
                                       "test ensemble), got %s" % sorted(labels))
            lab, ids = labels["labels"], labels.get("clip_ids")
        else:
            lab, ids = labels, None
        if self.test_meter is not None and ids is None:
            raise hip.SvitHipError("GraphedEvalStep(test_meter=...) needs the label tree {\"labels\", \"clip_ids\"}")
        if (self.val_meter is not None or self.test_meter is not None) and not torch.is_tensor(lab):
            raise hip.SvitHipError("the meters need the labels as an int64 [B] tensor")
        return lab, ids

    def refresh(self):
        """the bf16 copies of the weights, eagerly on the current stream (class docstring)"""
        with torch.no_grad():
            self.core.engine.refresh_weights()

    def _body(self, x, labels, mode):
        """mode "warm": the meters only fix their columns; "run": the captured body, and `eager`'s"""
        core = self.core
        eng = core.engine
        Tx = x.shape[2] if x.dim() == 5 else 1
        lab, ids = self._split(labels)
        y, _ = eng.forward(x, None, save=False)
        preds, extra = core.head_eval(y, Tx)
        if self.frames_pass and Tx > 1:       # B*T single frames through the same kernels (T' = 1)
            if self.frames_pass == "u8":      # (the clip forward above has run the RandAugment chain, if any)
                from .input import FramesView
                xf = FramesView(x, fresh=True)
            else:
                xf = x.transpose(1, 2).flatten(0, 1).unsqueeze(2)
            fy, _ = eng.forward(xf, None, save=False)
            fp, fe = core.head_eval(fy, 1)
            extra["frames_output"] = {"preds": fp, "extra_preds": fe}
        if self.val_meter is not None:
            from .train import eval_extra_metrics
            metrics = dict(eval_extra_metrics(self.cfg, preds, extra, lab, {}))
            if mode == "warm":
                self.val_meter.bind(metrics)
            else:
                self.val_meter.push(metrics, preds, lab, self.val_meter.ks)
        if self.test_meter is not None and mode != "warm":
            self.test_meter.update_stats(preds, lab, ids, repeat=self.repeat)
        return preds, extra

    def _capture(self, warmup):
        dev = self.x.device
        cap = torch.cuda.Stream(device=dev)
        cap.wait_stream(torch.cuda.current_stream(dev))
        with torch.no_grad():
            with torch.cuda.stream(cap):
                for _ in range(max(1, warmup)):       # lazy tables / library workspaces materialise here
                    self._body(self.x, self.labels, "warm")
            cap.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            # "thread_local": the process group's watchdog thread may query events while we capture
            with torch.cuda.graph(self.graph, stream=cap, capture_error_mode="thread_local"):
                self.preds, self.extra = self._body(self.x, self.labels, "run")
        torch.cuda.current_stream(dev).wait_stream(cap)
        torch.cuda.synchronize(dev)

    # ------------------------------------------------------------------------------------------
    def check_batch(self, inputs):
        """refuse a batch the capture does not fit (before anything is enqueued)"""
        x = inputs[0]
        if x.shape != self.x.shape:
            raise hip.SvitHipError("GraphedEvalStep was captured for input %s, got %s"
                                   % (tuple(self.x.shape), tuple(x.shape)))
        if torch.is_tensor(self.x) != torch.is_tensor(x) or (not torch.is_tensor(x) and type(x) is not type(self.x)):
            raise hip.SvitHipError("GraphedEvalStep was captured for a %s, got a %s"
                                   % (type(self.x).__name__, type(x).__name__))
        if not torch.is_tensor(x) and x.frames.shape != self.x.frames.shape:
            raise hip.SvitHipError("GraphedEvalStep was captured for a frame buffer %s, got %s: pad the batch to the "
                                   "captured size and pass the videos' extents"
                                   % (tuple(self.x.frames.shape), tuple(x.frames.shape)))

    def _host_half(self, n):
        if self.val_meter is not None:
            self.val_meter.host_update(n * getattr(self.wrapper, "world_size", 1), n)

    def _check_eval(self):
        if self.core.training:
            raise hip.SvitHipError("GraphedEvalStep runs the evaluation step: call model.eval() first")

    def __call__(self, inputs, labels):
        """-> (preds, extra): static tensors, overwritten by every replay"""
        self._check_eval()
        self.check_batch(inputs)
        x = inputs[0]
        if x.data_ptr() != self.x.data_ptr():
            self.x.copy_(x, non_blocking=True)        # (an AugClips: frames, records, extents)
        _tree_copy(self.labels, labels)
        self._host_half(self.x.shape[0])
        self.graph.replay()
        return self.preds, self.extra

    @torch.no_grad()
    def eager(self, inputs, labels):
        """the same body, uncaptured, on the given objects (any batch size: the short last batch of an epoch; the
        tests' twin) -> (preds, extra), fresh tensors"""
        self._check_eval()
        x = inputs[0]
        out = self._body(x, labels, "run")
        self._host_half(x.shape[0])
        return out

    @property
    def static_inputs(self):
        return [self.x]

    @property
    def static_labels(self):
        return self.labels


def _check_input_grad(cut):
    """GraphedTrainStep(input_grad=True) under a frozen cut: the captured backward would stop above the stem"""
    if cut > 0:
        raise hip.SvitHipError("GraphedTrainStep(input_grad=True) under a frozen cut (the parameters' requires_grad "
                               "flags freeze everything below position %d): the backward stops above the frozen blocks, "
                               "which keep no activations -- unfreeze the model for an input gradient" % cut)


def _check_ema(optimizer, ema, what):
    """refuse a replay after another ema.WeightEMA (or none) was attached to the optimizer than the step was built with"""
    if optimizer.ema is not ema:
        raise hip.SvitHipError("the optimizer's attached WeightEMA changed after this %s was built (%s then, %s now): its "
                               "tail holds the launches of then -- rebuild the step"
                               % (what, "one" if ema is not None else "none", "one" if optimizer.ema is not None else "none"))


def _check_monitor(optimizer, monitor, what):
    """refuse a replay after another monitor.TensorMonitor (or none) was attached to the optimizer than the step was built
    with"""
    if optimizer.monitor is not monitor:
        raise hip.SvitHipError("the optimizer's attached TensorMonitor changed after this %s was built (%s then, %s now): "
                               "its tail holds the launches of then -- rebuild the step"
                               % (what, "one" if monitor is not None else "none",
                                  "one" if optimizer.monitor is not None else "none"))


def _check_update_monitor(optimizer, monitor, what):
    """refuse a replay after another updmon.UpdateMonitor (or none) was attached to the optimizer than the step was built
    with"""
    if getattr(optimizer, "update_monitor", None) is not monitor:
        raise hip.SvitHipError("the optimizer's attached UpdateMonitor changed after this %s was built (%s then, %s now): "
                               "its tail holds the launches of then -- rebuild the step"
                               % (what, "one" if monitor is not None else "none",
                                  "one" if getattr(optimizer, "update_monitor", None) is not None else "none"))


def _check_act_monitor(core, monitor, what):
    """refuse a replay after another actmon.ActivationMonitor (or none) was attached to the model than the step was built
    with"""
    if core.engine.act_monitor is not monitor:
        raise hip.SvitHipError("the model's attached ActivationMonitor changed after this %s was built (%s then, %s now): "
                               "its forward holds the launches of then -- rebuild the step"
                               % (what, "one" if monitor is not None else "none",
                                  "one" if core.engine.act_monitor is not None else "none"))


def _check_attn_monitor(core, monitor, what):
    """refuse a replay after another attnmon.AttentionMonitor (or none) was attached to the model than the step was
    built with"""
    now = getattr(core.engine, "attn_monitor", None)
    if now is not monitor:
        raise hip.SvitHipError("the model's attached AttentionMonitor changed after this %s was built (%s then, %s now): "
                               "its forward holds the launches of then -- rebuild the step"
                               % (what, "one" if monitor is not None else "none", "one" if now is not None else "none"))


def _is_feeder(batch):
    from .feeder import ClipFeeder
    return isinstance(batch, ClipFeeder)


def _tree_map(fn, obj):
    if torch.is_tensor(obj):
        return fn(obj)
    if isinstance(obj, dict):
        return {k: _tree_map(fn, v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_tree_map(fn, v) for v in obj)
    return obj


def _tree_copy(dst, src):
    if torch.is_tensor(dst):
        if dst.data_ptr() != src.data_ptr():     # (the static buffer itself was handed back: nothing to copy)
            dst.copy_(src, non_blocking=True)
    elif isinstance(dst, dict):
        for k in dst:
            _tree_copy(dst[k], src[k])
    elif isinstance(dst, (list, tuple)):
        for d, s in zip(dst, src):
            _tree_copy(d, s)
