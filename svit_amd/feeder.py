"""The batch feeder: host batches -> the static buffers of a captured step, uploaded while the previous step runs.

Every stage of the uint8 route (augment.py, randaug.py, mixup.py, graph.py) works on a batch that already lies in device
memory.  This module is the boundary in front of it:

    step = GraphedTrainStep(model, loss_fun, [clips], labels, optimizer=opt, meter=meter)     # clips: an AugClips
    feeder = ClipFeeder.for_step(step)                          # depth=2 pinned + device slots, one copy stream
    feeder.put(videos, records, labels, randaug=table)          # HOST work only (a producer thread may call it)
    for _ in range(n):
        inputs, labels = feeder.next()                          # upload (if not yet under way) + ONE unpack launch
        step(inputs, labels)                                    # equal data_ptr()s: the step copies nothing
        feeder.pump()                                           # the next batch's upload runs beside this step

A SLOT is one batch as it travels: the videos packed TIGHTLY (`pack_tight`: video v as its own u8 [T,h_v,w_v,3], each
start rounded up to 16 bytes, no padding rows, nothing zeroed) and behind them, each part 16-byte aligned,

    frames | records int32 [B,16] | extents int32 [V,2] | RandAugment table int32 [V,N,16] | labels (leaf by leaf) | offsets int64 [V]

(parts the target does not have are absent; the offsets are the kernel's own table and stay in the slot).  `put` writes a
pinned slot, `pump` uploads the bytes in use with ONE host-to-device copy on the feeder's copy stream, and `next` launches
`svit_feed_unpack` (csrc/feed.hip) on the current stream: the videos into the top-left corners of the target's padded
buffer (`raw` under RandAugment, else `frames`; `fill` elsewhere) and the tables to where the step reads them.  After
`next` the target holds, byte for byte, what `AugClips(pack_videos(videos, Hs, Ws)[0].cuda(), ..., extents=, randaug=)`
would hold, so everything downstream is bit-equal to the direct route.

Ordering.  FIFO.  A pinned slot is rewritten only after the event behind its upload has completed (`next` waits for it
on the host -- it has to be complete before the step can run -- and hands the slot back to `put`); a device slot is
uploaded into only after the event behind its last unpack (a wait on the copy stream, not on the host).  Every GPU call
is made by the thread that calls `pump` / `next` / `close`; `put` and `wait` touch host memory and a lock only.

`unpack_host` is the NumPy restatement of the kernel's rules (include/svit_hip.h, svit_feed_unpack), wild tables
included: the kernel's yardstick, as `randaug.apply_host` is for RandAugment.

Out of scope: decoding and the dataset classes, `U8Clips` and fp32 tensors as targets, more than one producer thread,
uploads from inside the captured graph, compressed uploads, anything specific to more than one GPU.
"""
import collections
import threading
import time

import numpy as np
import torch

from . import hip
from .augment import AugClips, pack_extents, pack_records, validate_records

ALIGN = 16


class FeederFull(RuntimeError):
    """`put` found no free slot within its timeout"""


class FeederEmpty(RuntimeError):
    """`next` was called with nothing put"""


def _up(n, a=ALIGN):
    return (int(n) + a - 1) // a * a


def _as_video(x, v):
    """host u8 [T,h,w,3], torch or NumPy -> a C-contiguous NumPy view (a copy only of a non-contiguous one)"""
    if torch.is_tensor(x):
        if x.is_cuda:
            raise ValueError("video %d lives on the GPU: the feeder packs host memory" % v)
        x = x.numpy()
    x = np.asarray(x)
    if x.dtype != np.uint8 or x.ndim != 4 or x.shape[-1] != 3:
        raise ValueError("video %d: expected host uint8 [T,h,w,3], got %s %s" % (v, x.dtype, tuple(x.shape)))
    if x.shape[1] < 1 or x.shape[2] < 1:
        raise ValueError("video %d is empty: %s" % (v, tuple(x.shape)))
    return np.ascontiguousarray(x)


def tight_bytes(sizes, T):
    """bytes `pack_tight` uses for videos of these (h, w): each start rounded up to 16, the end too"""
    n = 0
    for h, w in sizes:
        n = _up(n) + int(T) * int(h) * int(w) * 3
    return _up(n)


def pack_tight(videos, out=None):
    """Videos of different sizes laid end to end.  videos: V host u8 [T,h_v,w_v,3], torch or NumPy, one T.  out: a 1-D
    uint8 host buffer to pack into (NumPy, or a torch tensor -- e.g. a pinned one), at least `tight_bytes` long; None
    allocates one.  -> (bytes, offsets, extents): `bytes` the used prefix of the buffer as a NumPy uint8 array (its
    length a multiple of 16), offsets int64 [V] the start of each video in it (multiples of 16, ascending), extents
    int32 [V,2] = (h_v, w_v).  Nothing is padded and nothing is zeroed: the up to 15 bytes between two videos keep
    whatever the buffer held."""
    if len(videos) == 0:
        raise ValueError("pack_tight needs at least one video")
    vids = [_as_video(x, v) for v, x in enumerate(videos)]
    T = vids[0].shape[0]
    for v, x in enumerate(vids):
        if x.shape[0] != T:
            raise ValueError("video %d has %d frames, video 0 has %d" % (v, x.shape[0], T))
    extents = np.array([[x.shape[1], x.shape[2]] for x in vids], dtype=np.int32)
    need = tight_bytes(extents.tolist(), T)
    if out is None:
        buf = np.empty(need, dtype=np.uint8)
    else:
        buf = out.numpy() if torch.is_tensor(out) else out
        if not isinstance(buf, np.ndarray) or buf.dtype != np.uint8 or buf.ndim != 1 or not buf.flags.c_contiguous:
            raise ValueError("out must be a contiguous 1-D uint8 host buffer")
        if buf.size < need:
            raise ValueError("out holds %d bytes, the batch needs %d" % (buf.size, need))
    offsets = np.empty(len(vids), dtype=np.int64)
    at = 0
    for v, x in enumerate(vids):
        at = _up(at)
        offsets[v] = at
        buf[at:at + x.size] = x.reshape(-1)
        at += x.size
    return buf[:need], offsets, extents


def unpack_host(slot, offsets, extents, T, Hs, Ws, fill=0, swap_rb=False, V=None):
    """What svit_feed_unpack writes into `frames`, in NumPy, for ANY tables.  slot: uint8 [slot_bytes]; offsets: int [V]
    or None (v*T*Hs*Ws*3); extents: int [V,2] or None (every video Hs x Ws); V: needed only when both are None.
    Per video (h, w) = the extent clamped into [1,Hs] x [1,Ws], n_v = T*h*w*3; offset < 0 or > slot_bytes - n_v: the
    video is absent, all `fill`; else frames[v,t,y,x,c] = slot[off + ((t*h + y)*w + x)*3 + (2-c if swap_rb else c)]
    inside the extent and `fill` outside.  -> uint8 [V,T,Hs,Ws,3].  Never indexes outside the slot."""
    slot = np.asarray(slot)
    if slot.dtype != np.uint8 or slot.ndim != 1:
        raise ValueError("the slot is uint8 [slot_bytes]")
    if not 0 <= int(fill) <= 255:
        raise ValueError("fill outside 0..255")
    nbytes = slot.size
    if offsets is not None:
        offsets = [int(o) for o in np.asarray(offsets).reshape(-1).tolist()]
        V = len(offsets)
    if extents is not None:
        extents = np.asarray(extents).reshape(-1, 2).tolist()
        V = len(extents) if V is None else V
        if len(extents) != V:
            raise ValueError("%d extents for %d offsets" % (len(extents), V))
    if V is None:
        raise ValueError("unpack_host needs offsets, extents or V")
    out = np.full((V, T, Hs, Ws, 3), int(fill), dtype=np.uint8)
    for v in range(V):
        h, w = (Hs, Ws) if extents is None else (min(max(int(extents[v][0]), 1), Hs), min(max(int(extents[v][1]), 1), Ws))
        n_v = T * h * w * 3                                   # (Python ints: the kernel's int64)
        off = v * T * Hs * Ws * 3 if offsets is None else offsets[v]
        if off < 0 or off > nbytes - n_v:
            continue
        assert 0 <= off and off + n_v <= nbytes
        vid = slot[off:off + n_v].reshape(T, h, w, 3)
        out[v, :, :h, :w] = vid[..., ::-1] if swap_rb else vid
    return out


def _leaves(tree):
    """the tensors of a label tree (a tensor, or dicts / lists / tuples of them) in iteration order"""
    if torch.is_tensor(tree):
        return [tree]
    if isinstance(tree, dict):
        return [t for k in tree for t in _leaves(tree[k])]
    if isinstance(tree, (list, tuple)):
        return [t for x in tree for t in _leaves(x)]
    return []


def _match_leaves(static, given, path="labels"):
    """the leaves of `given` that stand where `static` has tensors, in `_leaves` order"""
    if torch.is_tensor(static):
        return [(path, static, given)]
    if isinstance(static, dict):
        if not isinstance(given, dict):
            raise ValueError("%s: the step's labels are a dict, got %s" % (path, type(given).__name__))
        missing = [k for k in static if k not in given]
        if missing:
            raise ValueError("%s: missing %s" % (path, missing))
        return [m for k in static for m in _match_leaves(static[k], given[k], "%s[%r]" % (path, k))]
    if isinstance(static, (list, tuple)):
        if not isinstance(given, (list, tuple)) or len(given) != len(static):
            raise ValueError("%s: the step's labels are a sequence of %d" % (path, len(static)))
        return [m for i, (s, g) in enumerate(zip(static, given)) for m in _match_leaves(s, g, "%s[%d]" % (path, i))]
    return []


class SlotLayout:
    """Where the parts of a slot lie.  The frames come first and take what the batch needs; the small parts follow, each
    rounded up to 16 bytes: `parts` is an ordered list of (name, bytes).  `at(frames_bytes)` -> ({name: offset}, bytes in
    use); `slot_bytes` is the worst case, every video filling the buffer."""

    def __init__(self, V, T, Hs, Ws, parts):
        self.V, self.T, self.Hs, self.Ws = int(V), int(T), int(Hs), int(Ws)
        self.parts = [(str(n), int(b)) for n, b in parts]
        self.frames_max = tight_bytes([(Hs, Ws)] * self.V, T)
        self.slot_bytes = self.at(self.frames_max)[1]

    def at(self, frames_bytes):
        if frames_bytes < 0 or frames_bytes > self.frames_max:
            raise ValueError("%d frame bytes in a slot laid out for %d" % (frames_bytes, self.frames_max))
        off, where = _up(frames_bytes), {}
        for name, nbytes in self.parts:
            where[name] = off
            off = _up(off + nbytes)
        return where, max(off, ALIGN)


def layout_for(V, T, Hs, Ws, B, randaug_layers=0, extents=True, label_bytes=()):
    """the SlotLayout of a target with B records, a RandAugment table of `randaug_layers` layers (0: none), with or
    without an extents table, and label leaves of these sizes in bytes"""
    parts = [("records", B * 64)]
    if extents:
        parts.append(("extents", V * 8))
    if randaug_layers:
        parts.append(("randaug", V * randaug_layers * 64))
    parts += [("labels%d" % i, n) for i, n in enumerate(label_bytes)]
    parts.append(("offsets", V * 8))
    return SlotLayout(V, T, Hs, Ws, parts)


class _Slot:
    def __init__(self, host, dev):
        self.host, self.host_np, self.dev = host, host.numpy(), dev
        self.h2d, self.done = torch.cuda.Event(), torch.cuda.Event()
        self.unpacked = False            # `done` has been recorded at least once
        self.where, self.used, self.args = None, 0, None


class ClipFeeder:
    """Host batches -> the static AugClips of a captured step (module docstring).
    target: the AugClips the step was captured over (`step.static_inputs[0]`), with or without RandAugment and with or
    without extents -- without extents every video must be exactly Hs x Ws.  labels: `step.static_labels`, a tensor or a
    tree of tensors (the image rank's dict).  depth: slots in the ring (pinned host + device, `slot_bytes` each).
    swap_rb / fill: svit_feed_unpack's (fill=0, swap_rb=False reproduce `pack_videos`)."""

    def __init__(self, target, labels, depth=2, swap_rb=False, fill=0):
        if not isinstance(target, AugClips):
            raise hip.SvitHipError("ClipFeeder feeds an augment.AugClips, got %s" % type(target).__name__)
        if depth < 1:
            raise ValueError("depth must be at least 1")
        if not 0 <= int(fill) <= 255:
            raise ValueError("fill outside 0..255")
        self.target, self.labels = target, labels
        self.depth, self.swap_rb, self.fill = int(depth), bool(swap_rb), int(fill)
        self._dst = target.frames if target.raw is None else target.raw
        self.device = self._dst.device
        V, T, Hs, Ws, _ = self._dst.shape
        self._label_leaves = _leaves(labels)
        for t in self._label_leaves:
            if t.device != self.device or not t.is_contiguous():
                raise hip.SvitHipError("the static labels must be contiguous tensors on %s" % (self.device,))
        self.layout = layout_for(V, T, Hs, Ws, target.records.shape[0],
                                 0 if target.ra_table is None else target.ra_table.shape[1], target.extents is not None,
                                 [t.numel() * t.element_size() for t in self._label_leaves])
        if len(self.layout.parts) - 1 > 8:
            raise hip.SvitHipError("the target has %d tables and label tensors; one unpack launch carries 8"
                                   % (len(self.layout.parts) - 1))
        self.slot_bytes = self.layout.slot_bytes
        self._slots = [_Slot(torch.empty(self.slot_bytes, dtype=torch.uint8).pin_memory(),
                             torch.empty(self.slot_bytes, dtype=torch.uint8, device=self.device))
                       for _ in range(self.depth)]
        self._copy = torch.cuda.Stream(device=self.device)
        self._cv = threading.Condition()
        self._free = collections.deque(range(self.depth))      # pinned slots `put` may write
        self._filled = collections.deque()                      # packed, not yet uploaded (FIFO)
        self._uploaded = collections.deque()                    # upload enqueued, not yet unpacked (FIFO)
        self._closed = False

    @classmethod
    def for_step(cls, step, **kw):
        """the feeder of a GraphedTrainStep captured over an AugClips"""
        return cls(step.static_inputs[0], step.static_labels, **kw)

    # ---- the producer's side: host memory and the lock only -----------------------------------------------------------
    def _check(self, videos, records, labels, randaug):
        tgt = self.target
        V, T, Hs, Ws, _ = self._dst.shape
        if len(videos) != V:
            raise ValueError("the target holds %d videos, got %d" % (V, len(videos)))
        vids = [_as_video(x, v) for v, x in enumerate(videos)]
        for v, x in enumerate(vids):
            if x.shape[0] != T:
                raise ValueError("video %d has %d frames, the target %d" % (v, x.shape[0], T))
        sizes = [[x.shape[1], x.shape[2]] for x in vids]
        ext = None
        if tgt.extents is not None:
            ext = pack_extents(np.array(sizes, dtype=np.int64), V, Hs, Ws, tgt._min_side)
        else:
            for v, (h, w) in enumerate(sizes):
                if (h, w) != (Hs, Ws):
                    raise ValueError("video %d is %dx%d; a target without extents takes exactly %dx%d" % (v, h, w, Hs, Ws))
        table = pack_records(records)
        if table.is_cuda:
            raise ValueError("the records of a fed batch are host data")
        if table.shape != tgt.records.shape:
            raise ValueError("the record table is int32 %s, got %s" % (tuple(tgt.records.shape), tuple(table.shape)))
        validate_records(table, V, Hs, Ws, tgt.size, ext)       # host tensors: no device synchronisation
        ra = None
        if tgt.ra_table is not None:
            if randaug is None:
                raise ValueError("the target runs RandAugment: put(..., randaug=table)")
            ra = tgt._pack_randaug(randaug)
            if ra.is_cuda or ra.shape != tgt.ra_table.shape:
                raise ValueError("the RandAugment table is host int32 %s, got %s" % (tuple(tgt.ra_table.shape), tuple(ra.shape)))
        elif randaug is not None:
            raise ValueError("the target was built without RandAugment")
        leaves = []
        for path, static, given in _match_leaves(self.labels, labels):
            g = torch.as_tensor(given)
            if g.is_cuda:
                raise ValueError("%s: the labels of a fed batch are host data" % path)
            if g.shape != static.shape:
                raise ValueError("%s: the step holds %s, got %s" % (path, tuple(static.shape), tuple(g.shape)))
            leaves.append(g.to(static.dtype).contiguous().reshape(-1).view(torch.uint8).numpy())
        return vids, sizes, ext, table, ra, leaves

    def put(self, videos, records, labels, randaug=None, timeout=None):
        """Pack one batch into a free pinned slot (host work only; one producer thread).  videos: V host u8
        [T,h_v,w_v,3]; records: B AugRecord (or int32 [B,16]), validated against their own videos; labels: what the
        step's static labels hold, as host tensors / arrays of the same tree; randaug: the [V,N,16] table (or lists of
        RandAugOp) when the target runs RandAugment.  No free slot: waits up to `timeout` seconds (None: until one is
        free, 0: not at all), then raises FeederFull."""
        vids, sizes, ext, table, ra, leaves = self._check(videos, records, labels, randaug)
        end = None if timeout is None else time.monotonic() + timeout
        with self._cv:
            while not self._free:
                if self._closed:
                    raise RuntimeError("the feeder is closed")
                left = None if end is None else end - time.monotonic()
                if left is not None and left <= 0:
                    raise FeederFull("all %d slots hold batches that have not been consumed" % self.depth)
                self._cv.wait(left)
            if self._closed:
                raise RuntimeError("the feeder is closed")
            i = self._free.popleft()
        s = self._slots[i]
        buf = s.host_np
        used, offsets, _ = pack_tight(vids, out=buf)
        where, total = self.layout.at(used.size)

        def write(name, arr):
            b = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
            buf[where[name]:where[name] + b.size] = b
        write("records", table.numpy())
        if ext is not None:
            write("extents", ext.numpy())
        if ra is not None:
            write("randaug", ra.numpy())
        for k, leaf in enumerate(leaves):
            write("labels%d" % k, leaf)
        write("offsets", offsets)
        s.where, s.used = where, total
        with self._cv:
            self._filled.append(i)
            self._cv.notify_all()

    def wait(self, timeout=None):
        """block (host only) until a batch has been put and not yet consumed -> whether there is one"""
        with self._cv:
            self._cv.wait_for(lambda: self._filled or self._uploaded or self._closed, timeout)
            return bool(self._filled or self._uploaded) and not self._closed

    @property
    def pending(self):
        """batches put and not yet handed out by `next`"""
        with self._cv:
            return len(self._filled) + len(self._uploaded)

    # ---- the consumer's side: every GPU call ----------------------------------------------------------------------------
    def pump(self):
        """enqueue the upload of every packed slot on the copy stream (behind the slot's last unpack) -> how many"""
        n = 0
        while True:
            with self._cv:
                if not self._filled:
                    return n
                i = self._filled.popleft()
            s = self._slots[i]
            if s.unpacked:
                self._copy.wait_event(s.done)                   # the device slot's last reader
            with torch.cuda.stream(self._copy):
                s.dev[:s.used].copy_(s.host[:s.used], non_blocking=True)
                s.h2d.record(self._copy)
            with self._cv:
                self._uploaded.append(i)
            n += 1

    def _args(self, s):
        from . import ops
        tgt, w = self.target, s.where
        segs = [(w["records"], tgt.records)]
        if tgt.extents is not None:
            segs.append((w["extents"], tgt.extents))
        if tgt.ra_table is not None:
            segs.append((w["randaug"], tgt.ra_table))
        segs += [(w["labels%d" % k], t) for k, t in enumerate(self._label_leaves)]
        V = self._dst.shape[0]
        offsets = s.dev[w["offsets"]:w["offsets"] + V * 8].view(torch.int64)
        extents = None if tgt.extents is None else s.dev[w["extents"]:w["extents"] + V * 8].view(torch.int32).view(V, 2)
        return ops.feed_args(s.dev, self._dst, offsets, extents, self.fill, self.swap_rb, segs, slot_bytes=s.used)

    def next(self):
        """The oldest batch into the target: `pump()`, the current stream waits for that slot's upload, ONE
        svit_feed_unpack launch.  -> ([target], labels), the step's own static objects.  FeederEmpty when nothing was put."""
        from . import ops
        self.pump()
        with self._cv:
            if not self._uploaded:
                raise FeederEmpty("next() on a feeder nothing was put into")
            i = self._uploaded.popleft()
        s = self._slots[i]
        main = torch.cuda.current_stream(self.device)
        main.wait_event(s.h2d)
        s.args = self._args(s)                                  # (kept: the launch reads the struct, not the tensors)
        ops.feed_unpack(s.args)
        s.done.record(main)
        s.unpacked = True
        s.h2d.synchronize()          # the upload has read the pinned slot: `put` may rewrite it
        with self._cv:
            self._free.append(i)
            self._cv.notify_all()
        return [self.target], self.labels

    def close(self):
        """wake a blocked `put`, wait for the feeder's copies and launches, free the slots"""
        with self._cv:
            if self._closed:
                return
            self._closed = True
            self._cv.notify_all()
        self._copy.synchronize()
        for s in self._slots:
            if s.unpacked:
                s.done.synchronize()
        self._slots = []
        self._free.clear()
        self._filled.clear()
        self._uploaded.clear()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Producer(threading.Thread):
    """One thread that drains an iterable of `put` argument tuples (videos, records, labels[, randaug]) into a feeder,
    as far ahead as the ring has free slots.  Host work only.  `wait_ready()` (consumer) blocks until a batch is there
    and re-raises what the iterable or `put` raised; `stop()` ends it."""

    def __init__(self, feeder, batches):
        super().__init__(name="svit-feeder-producer", daemon=True)
        self.feeder, self.batches = feeder, batches
        self.error, self.finished, self._stop_flag = None, False, False

    def run(self):
        try:
            for args in self.batches:
                while not self._stop_flag:
                    try:
                        self.feeder.put(*args, timeout=0.05)
                        break
                    except FeederFull:
                        continue
                if self._stop_flag:
                    break
        except BaseException as e:              # handed to the consumer
            self.error = e
        finally:
            self.finished = True
            with self.feeder._cv:
                self.feeder._cv.notify_all()

    def wait_ready(self):
        f = self.feeder
        with f._cv:
            f._cv.wait_for(lambda: f._filled or f._uploaded or self.finished or f._closed)
            ready = bool(f._filled or f._uploaded)
        if not ready:
            if self.error is not None:
                err, self.error = self.error, None
                raise err
            raise FeederEmpty("the producer has ended and every batch has been consumed")

    def stop(self):
        self._stop_flag = True
        self.join()
        if self.error is not None:
            err, self.error = self.error, None
            raise err
