"""oracle/dropout_np.py — the host restatement of the fused small-batch step's dropout masks (csrc/hgin_smallbatch.hip
drop_factor) — against the published splitmix64 sequence, a second implementation on Python's unbounded integers, the
threshold arithmetic of hgin/smallbatch.py, and the properties the GPU tests (tests/test_gpu_dropmask.py) lean on:
masks separate by layer, type, step and seed, do not depend on a block's row count, and drop a share p."""
import math

import numpy as np
import pytest

from oracle import dropout_np as dn

M64 = 2 ** 64 - 1


def _hash_int(seed: int, ctr: int, l: int, t: int, q: int) -> int:
    """The same function on Python integers, every step reduced modulo 2^64 by masking."""
    x = (seed + ctr * 0x9E3779B97F4A7C15) & M64
    x ^= (((l * 3 + t) << 56) & M64) ^ q
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def test_raw_hash_is_splitmix64():
    """seed = l = t = q = 0: the hashes at ctr = 1, 2, 3 are splitmix64's first outputs from state 0."""
    want = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert [int(dn.raw_hash(0, c, 0, 0, 0)) for c in (1, 2, 3)] == want
    assert [int(v) for v in dn.raw_hash(0, np.array([1, 2, 3]), 0, 0, 0)] == want
    assert [_hash_int(0, c, 0, 0, 0) for c in (1, 2, 3)] == want
    # thr = 0 keeps everything, whatever the hash
    assert dn.drop_threshold(0.0) == 0 and dn.keep_mask(0, 1, 0, 0, 5, 3, 0.0).all()


def test_numpy_equals_python_int_version():
    rng = np.random.default_rng(20240607)
    n = 4096
    seed = rng.integers(0, 2 ** 62, n, dtype=np.int64)
    ctr = rng.integers(0, 2 ** 40, n, dtype=np.int64)
    ctr[: n // 4] = rng.integers(0, 64, n // 4)          # the counters a test run sees
    l = rng.integers(0, 3, n)
    t = rng.integers(0, 3, n)
    q = rng.integers(0, 2 ** 31, n, dtype=np.int64)
    q[:8] = [0, 1, 2 ** 31 - 1, 2 ** 31 - 2, 127, 128, 2 ** 16, 2 ** 24 + 1]
    got = dn.raw_hash(seed, ctr, l, t, q)
    assert got.dtype == np.uint64
    want = [_hash_int(int(s), int(c), int(a), int(b), int(e)) for s, c, a, b, e in zip(seed, ctr, l, t, q)]
    assert [int(v) for v in got] == want
    # seed + ctr * golden past 2^64: with these seeds any ctr >= 2 wraps; assert that the sample has both kinds
    wraps = np.array([int(s) + int(c) * dn.GOLDEN > M64 for s, c in zip(seed, ctr)])
    assert wraps.sum() > 1000 and (~wraps).sum() > 10
    # and the largest seed the step draws with the smallest wrapping counter, by hand
    s, c = 2 ** 62 - 1, 2
    assert s + c * dn.GOLDEN > M64
    assert int(dn.raw_hash(s, c, 2, 2, 2 ** 31 - 1)) == _hash_int(s, c, 2, 2, 2 ** 31 - 1)
    # keep_mask is the threshold on the top 32 bits of exactly this hash, q = i * H + h
    m = dn.keep_mask(int(seed[0]), 7, 1, 2, 13, 24, 0.3)
    assert m.shape == (13, 24) and m.dtype == np.bool_
    for i, h in ((0, 0), (0, 23), (1, 0), (12, 23), (5, 7)):
        assert bool(m[i, h]) == ((_hash_int(int(seed[0]), 7, 1, 2, i * 24 + h) >> 32) >= 1288490189)


def test_thresholds_and_scale():
    assert dn.drop_threshold(0.3) == 1288490189
    assert dn.drop_threshold(0.1) == 429496730
    assert dn.drop_threshold(0.5) == 2147483648
    assert dn.drop_threshold(1.0 - 2.0 ** -40) == 2 ** 32 - 1   # just under 1: round() reaches 2^32, clamped
    assert dn.drop_threshold(math.nextafter(1.0, 0.0)) == 2 ** 32 - 1
    for p in (0.1, 0.3, 0.5):
        assert dn.drop_scale(p) == float(np.float32(1.0 / (1.0 - p)))
    assert dn.drop_scale(0.5) == 2.0 and dn.drop_scale(0.3) != 1.0 / 0.7   # (float32, not float64)


def test_masks_separate_and_ignore_the_row_count():
    seed, ctr, rows, H, p = 0x1234_5678_9ABC_DEF0 >> 2, 5, 37, 24, 0.3
    base = dn.keep_mask(seed, ctr, 1, 1, rows, H, p)
    others = {"l": dn.keep_mask(seed, ctr, 0, 1, rows, H, p), "l2": dn.keep_mask(seed, ctr, 2, 1, rows, H, p),
              "t": dn.keep_mask(seed, ctr, 1, 0, rows, H, p), "t2": dn.keep_mask(seed, ctr, 1, 2, rows, H, p),
              "ctr": dn.keep_mask(seed, ctr + 1, 1, 1, rows, H, p), "seed": dn.keep_mask(seed + 1, ctr, 1, 1, rows, H, p),
              # (l, t) enters as 3 l + t: (0, 3) does not exist, but (1, 0) and (0, 2) + 1 must not alias either
              "lt": dn.keep_mask(seed, ctr, 0, 2, rows, H, p)}
    for k, m in others.items():
        # independent masks at p = 0.3 disagree on a share 2 p (1 - p) = 0.42 of 888 elements
        assert 0.3 < float((m != base).mean()) < 0.54, k
    masks = [base] + list(others.values())
    for i in range(len(masks)):
        for j in range(i):
            assert not np.array_equal(masks[i], masks[j]), (i, j)
    assert np.array_equal(dn.keep_mask(seed, ctr, 1, 1, rows + 7, H, p)[:rows], base)


def test_activation_yardsticks_are_the_float32_oracles_own_error():
    """tests/test_gpu_dropmask.py bounds every (layer, type) block of the step's layer outputs by 8 x a recorded ratio
    per case: torch's own float32 evaluation of the oracle against its float64 evaluation under the same host masks on
    the same batch (tests/smallbatch_cases.py fp32_act_ratio).  Recomputed here, the recorded figures hold within a
    quarter (a float32 GEMM's summation order, and with it the last digit of every sum, depends on the host's BLAS
    blocking and thread count; the worst block's norm ratio over thousands of elements moves by a few percent)."""
    import copy

    import torch

    import smallbatch_cases as sc
    import test_gpu_dropmask as T
    from hgin import HetroGIN
    b = sc.store_host_batch(sc.store_graphs(**T.GIN_STORE), T.GIN_IDS)
    for hidden, layers, p, ratio in T.GIN_CASES:
        kw = sc.model_kwargs(node_embedding_size=hidden, message_passing_layers=layers, dropout=p)
        torch.manual_seed(1997)
        m = HetroGIN(**dict(kw, input_channels=dict(kw["input_channels"])))
        got = sc.fp32_act_ratio(lambda dt: sc.oracle_twin(m, kw, dt), b, p, hidden)
        assert ratio / 1.25 <= got <= ratio * 1.25, (hidden, layers, p, got, ratio)
    b = sc.store_host_batch(sc.store_graphs(**T.GAT_STORE), T.GAT_IDS)
    for heads, C, ratio in T.GAT_CASES:
        base = sc.glorot_gat_oracle(sc.gat_kwargs(heads=heads, node_embedding_size=C, dropout=0.3))
        got = sc.fp32_act_ratio(lambda dt: copy.deepcopy(base).to(dt), b, 0.3, heads * C)
        assert ratio / 1.25 <= got <= ratio * 1.25, (heads, C, got, ratio)


@pytest.mark.parametrize("p", [0.1, 0.3, 0.5])
def test_drop_rate(p):
    """2^20 elements of one fixed seed: the dropped share within 4 binomial standard deviations of p."""
    n = 2 ** 20
    m = dn.keep_mask(0x2545F4914F6CDD1D >> 2, 3, 1, 0, n // 64, 64, p)
    assert m.size == n
    share = 1.0 - float(m.mean())
    assert abs(share - p) <= 4.0 * math.sqrt(p * (1.0 - p) / n), (p, share)
