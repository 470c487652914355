"""Host side of the guarded optimizer tail (svit_step_guard / svit_adamw_step_guarded / svit_adamw_bias_table,
optim.GuardedClipAdamW): the bias-correction table against glibc, the step record's layout, argument validation and
the choice construct_optimizer makes.  No GPU needed."""
import ctypes as C
import types

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from svit_amd import hip
    return hip.load()


_libm = C.CDLL("libm.so.6")
_libm.powf.restype = _libm.sqrtf.restype = C.c_float
_libm.powf.argtypes = [C.c_float, C.c_float]
_libm.sqrtf.argtypes = [C.c_float]


def _glibc_pair(beta1, beta2, step):
    """svit_adamw_step's expression, evaluated in float32 through glibc"""
    one = np.float32(1.0)
    bc1 = one - np.float32(_libm.powf(beta1, float(step)))
    bc2 = np.float32(_libm.sqrtf(one - np.float32(_libm.powf(beta2, float(step)))))
    return np.float32(bc1), bc2


@pytest.mark.parametrize("betas,length", [((0.9, 0.999), 17321), ((0.9, 0.95), 338), ((0.9, 0.9999), 173250)])
def test_bias_table_is_glibc_bit_for_bit(lib, betas, length):
    from svit_amd import ops
    t = ops.adamw_bias_table(*betas)
    assert t.dtype == np.float32 and t.shape == (length, 2)
    ref = np.empty((length, 2), dtype=np.float32)
    for k in range(1, length + 1):
        ref[k - 1] = _glibc_pair(betas[0], betas[1], k)
    assert np.array_equal(t.view(np.uint32), ref.view(np.uint32))
    assert tuple(t[-1]) == (1.0, 1.0)
    assert tuple(t[-2]) != (1.0, 1.0)
    # the length alone (no table), and a table that is too short
    n = C.c_int64(0)
    assert lib.svit_adamw_bias_table(betas[0], betas[1], None, 0, C.byref(n)) == 0 and n.value == length
    short = np.empty((length - 1, 2), dtype=np.float32)
    assert lib.svit_adamw_bias_table(betas[0], betas[1], short.ctypes.data, length - 1, C.byref(n)) == -4


def test_bias_table_refuses_more_than_2_pow_20_entries(lib):
    from svit_amd import hip, ops
    n = C.c_int64(0)
    assert lib.svit_adamw_bias_table(0.9, 0.9999999, None, 0, C.byref(n)) == -4
    assert lib.svit_adamw_bias_table(0.9, 0.999, None, 0, None) == -4
    with pytest.raises(hip.SvitHipError):
        ops.adamw_bias_table(0.9, 0.9999999)


def test_step_record_layout_and_packer(lib):
    """sizes and offsets as include/svit_hip.h states them; pack_step_host's bytes read back through the structure"""
    from svit_amd import hip
    from svit_amd.optim import pack_step_host
    H, D = hip.StepHost, hip.StepDev
    assert C.sizeof(H) == 32 and C.sizeof(D) == 48
    assert [(n, getattr(H, n).offset) for n, _ in H._fields_] == [
        ("lr", 0), ("weight_decay", 8), ("max_norm", 16), ("clip_value", 20), ("grad_scale", 24), ("reserved", 28)]
    assert [(n, getattr(D, n).offset) for n, _ in D._fields_] == [
        ("applied", 0), ("skipped", 8), ("consecutive", 16), ("apply", 20), ("coef", 24), ("bc1", 28),
        ("bc2_sqrt", 32), ("sumsq", 36), ("grad_norm", 40), ("reserved", 44)]
    raw = pack_step_host((1e-3, 2e-3), (0.05, 0.0), 1.0, None, 0.5)
    assert raw.dtype == np.float32 and raw.nbytes == 32
    h = H.from_buffer_copy(raw.tobytes())
    f = np.float32
    assert (h.lr[0], h.lr[1]) == (f(1e-3), f(2e-3)) and (h.weight_decay[0], h.weight_decay[1]) == (f(0.05), f(0.0))
    assert (h.max_norm, h.clip_value, h.grad_scale, h.reserved) == (1.0, 0.0, 0.5, 0.0)
    # a clip value switches norm clipping off (tools/train_net.py:139-147 of the reference: value before norm)
    h = H.from_buffer_copy(pack_step_host((1e-3, 1e-3), (0.05, 0.0), 1.0, 0.01, 1.0).tobytes())
    assert (h.max_norm, h.clip_value) == (0.0, f(0.01))
    # what the kernels read is what the host would read
    d = D()
    d.applied, d.skipped, d.consecutive, d.grad_norm = (1 << 40) + 3, 7, 2, 1.5
    words = np.frombuffer(bytes(d), dtype=np.int32)
    assert words.size == 12 and int(words[:2].view(np.int64)[0]) == (1 << 40) + 3
    assert int(words[2:4].view(np.int64)[0]) == 7 and words[4] == 2 and words[10:11].view(np.float32)[0] == 1.5


def test_guarded_argument_validation_without_gpu(lib):
    """bad calls are refused before any launch (stream = None, made-up pointers that are never followed)"""
    P = 4096          # any 16-byte aligned non-null address
    assert lib.svit_step_guard(None, 100, P, P, P, 10, P, 1024, None) == -4
    assert lib.svit_step_guard(P, 100, None, P, P, 10, P, 1024, None) == -4
    assert lib.svit_step_guard(P, 100, P, None, P, 10, P, 1024, None) == -4
    assert lib.svit_step_guard(P, 100, P, P, None, 10, P, 1024, None) == -4        # entries without a table
    assert lib.svit_step_guard(P, 100, P, P, P, 10, None, 1024, None) == -4
    assert lib.svit_step_guard(P, 0, P, P, P, 10, P, 1024, None) == -4
    assert lib.svit_step_guard(P, -5, P, P, P, 10, P, 1024, None) == -4
    assert lib.svit_step_guard(P, 100, P, P, P, -1, P, 1024, None) == -4
    assert lib.svit_step_guard(P, 100, P, P, P, 10, P, 0, None) == -4              # no room for one partial
    assert lib.svit_step_guard(P, 100, P + 4, P, P, 10, P, 1024, None) == -3       # record not 8-byte aligned
    assert lib.svit_step_guard(P, 100, P, P + 4, P, 10, P, 1024, None) == -3
    a = (0.9, 0.999, 1e-8, None)
    for i in range(4):                                                            # p, g, m, v
        ptrs = [P, P, P, P]
        ptrs[i] = None
        assert lib.svit_adamw_step_guarded(*ptrs, 100, 50, P, P, *a) == -4
        ptrs[i] = P + 4
        assert lib.svit_adamw_step_guarded(*ptrs, 100, 50, P, P, *a) == -3
    assert lib.svit_adamw_step_guarded(P, P, P, P, 100, 50, None, P, *a) == -4
    assert lib.svit_adamw_step_guarded(P, P, P, P, 100, 50, P, None, *a) == -4
    assert lib.svit_adamw_step_guarded(P, P, P, P, 0, 0, P, P, *a) == -4
    assert lib.svit_adamw_step_guarded(P, P, P, P, -1, 0, P, P, *a) == -4
    assert lib.svit_adamw_step_guarded(P, P, P, P, 100, 101, P, P, *a) == -4       # n_decay > n
    assert lib.svit_adamw_step_guarded(P, P, P, P, 100, -1, P, P, *a) == -4
    assert lib.svit_adamw_step_guarded(P, P, P, P, 100, 50, P + 4, P, *a) == -3


class _StubFlat:
    """what FusedClipAdamW touches of a model's FlatParams, on the CPU"""

    def __init__(self, n=37, n_decay=20):
        self.total, self.n_decay = n, n_decay
        self.data = torch.zeros(n)
        self.grad = torch.zeros(n)


def _stub_cfg(**solver):
    from svit_amd import config
    cfg = config.ssv2_cfg(num_frames=4, crop=64)
    for k, v in solver.items():
        setattr(cfg.SOLVER, k, v)
    return cfg


def test_construct_optimizer_selection(lib):
    from svit_amd import optim
    model = types.SimpleNamespace(flat=_StubFlat())
    cfg = _stub_cfg()
    assert cfg.SOLVER.CLIP_GRAD_VAL is None and not hasattr(cfg.SVIT, "GUARDED_STEP")
    classic = optim.construct_optimizer(model, cfg)
    assert type(classic) is optim.FusedClipAdamW

    cfg = _stub_cfg()
    cfg.SVIT.GUARDED_STEP = True
    g = optim.construct_optimizer(model, cfg)
    assert type(g) is optim.GuardedClipAdamW
    assert g.clip == cfg.SOLVER.CLIP_GRAD_L2NORM and g.clip_value is None and g.max_consecutive_skips is None
    assert g.bias_table.shape == (17321, 2)
    assert [tuple(x["range"]) for x in g.param_groups] == [(0, 20), (20, 37)]
    assert g.step_count == 0
    g.step_count = 5                       # the record holds it (checkpoint loading writes it the same way)
    assert g.step_count == 5 and g.stats()["applied"] == 5 and g.stats()["skipped"] == 0
    optim.set_lr(g, 0.25)                  # set_lr reaches the next upload
    assert g._pack()[0] == np.float32(0.25) and g._pack()[1] == np.float32(0.25)
    g.check()                              # no limit: never raises

    cfg = _stub_cfg(CLIP_GRAD_VAL=0.5)
    g = optim.construct_optimizer(model, cfg)
    assert type(g) is optim.GuardedClipAdamW and g.clip_value == 0.5
    h = g._pack()
    assert h[4] == 0.0 and h[5] == np.float32(0.5)      # value clipping replaces norm clipping

    cfg = _stub_cfg()
    cfg.SVIT.GUARDED_STEP = False
    assert type(optim.construct_optimizer(model, cfg)) is optim.FusedClipAdamW
