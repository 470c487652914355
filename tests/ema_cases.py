"""Shared cases of the weight-EMA tests (tests/test_ema_cpu.py, tests/test_ema_gpu.py): the range tables of the kernel
checks, the closed form of the warm-up table written out independently of the library, and the float64 yardstick."""
import numpy as np

N = 8 * 1024 + 11               # eight windows of 1024 floats and a ninth of 11: n % 4 = 3
N4 = N // 4 * 4

# the kernel's range tables at n = N (every bound a multiple of 4)
TABLES = {
    "one range": [[0, N4]],
    "window edges": [[0, 1024], [1024, 2048], [2048, 4096], [5120, 6144], [7168, N4]],
    # 4, 8 and 12 floats inside the window [1024, 2048)
    "three in a window": [[0, 8], [1028, 1032], [1040, 1048], [1100, 1112], [4000, 5000]],
    # every range begins where the one before ends; reaches the last whole quad
    "touching": [[0, 512], [512, 516], [516, 2048], [2048, 2052], [2052, N4]],
    # the limit: 64 ranges of 4 .. 20 floats
    "64 ranges": [[128 * i, 128 * i + 4 * (1 + i % 5)] for i in range(64)],
}


def segs(rows):
    return np.ascontiguousarray(np.array(rows, dtype=np.int64).reshape(-1, 2))


def inside(rows, n=N):
    m = np.zeros(n, dtype=bool)
    for a, b in rows:
        assert not m[a:b].any(), "ranges overlap"
        m[a:b] = True
    return m


def warmup_closed_form(decay, k):
    """entry k - 1 of the warm-up table: (float) min((double) decay, (1 + k) / (10 + k)), k an int or an int array"""
    k = np.asarray(k, dtype=np.float64)
    return np.minimum(np.float64(np.float32(decay)), (1.0 + k) / (10.0 + k)).astype(np.float32)


def warmup_length(decay):
    """the first k whose entry equals float32(decay), by linear search from the real-valued crossing"""
    d = np.float32(decay)
    k = max(1, int((10.0 * float(d) - 1.0) / (1.0 - float(d))) - 2000)
    while warmup_closed_form(decay, k) != d:
        k += 1
    assert k == 1 or warmup_closed_form(decay, k - 1) != d
    return k


def same_np(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))
