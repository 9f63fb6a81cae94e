"""ORACLE — test infrastructure only.  numpy restatement of the fused small-batch step's dropout masks
(``csrc/hgin_smallbatch.hip`` ``drop_factor``; ``hgin/smallbatch.py`` sets ``drop_seed`` / ``drop_thr`` / ``drop_inv``).

Only ``tests/`` may import it.  It states the generator from its definition, not from the kernel's code:

* the step keeps a 64-bit seed (drawn once per ``SmallBatchStep``) and a step counter ``ctr`` that the step's last
  launch advances by one, so step k of a fresh ``SmallBatchStep`` (its warm-up steps included) reads ``ctr = k``;
* element ``q = row * H + column`` of layer ``l``'s output of node type ``t`` (0 / 1 / 2 = path / link / node, the
  order of ``act_off``) has the 64-bit hash ``mix(seed + ctr * GOLDEN ^ ((3 l + t) << 56) ^ q)``, all in arithmetic
  modulo 2^64, where ``GOLDEN`` = 0x9E3779B97F4A7C15 is splitmix64's increment and ``mix`` its output finaliser
  (xor-shift 30, multiply 0xBF58476D1CE4E5B9, xor-shift 27, multiply 0x94D049BB133111EB, xor-shift 31): with
  ``seed = l = t = q = 0`` the hashes at ``ctr = 1, 2, 3, ...`` are the published splitmix64 sequence of seed 0;
* the element is dropped when the hash's top 32 bits are below ``round(p 2^32)`` (clamped to 2^32 - 1), and a kept
  element is scaled by ``1 / (1 - p)`` rounded to float32.

The row count of a block does not enter: a type's capacity-sized block and its valid rows share their leading masks.
"""
from __future__ import annotations

import numpy as np

GOLDEN = 0x9E3779B97F4A7C15
MIX1 = 0xBF58476D1CE4E5B9
MIX2 = 0x94D049BB133111EB


def drop_threshold(p: float) -> int:
    """``drop_thr``: an element is dropped when the top 32 bits of its hash are below this."""
    return min(int(round(float(p) * 2 ** 32)), 2 ** 32 - 1)


def drop_scale(p: float) -> float:
    """``drop_inv``: 1 / (1 - p) as the step's float32 field holds it."""
    return float(np.float32(1.0 / (1.0 - float(p))))


def raw_hash(seed, ctr, l, t, q) -> np.ndarray:
    """The 64-bit hash (uint64) before the threshold; the arguments broadcast against each other."""
    u = lambda v: np.asarray(v).astype(np.uint64)   # noqa: E731
    with np.errstate(over="ignore"):
        x = u(seed) + u(ctr) * np.uint64(GOLDEN)
        x = x ^ ((u(l) * np.uint64(3) + u(t)) << np.uint64(56)) ^ u(q)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(MIX1)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(MIX2)
        return x ^ (x >> np.uint64(31))


def keep_mask(seed: int, ctr: int, l: int, t: int, rows: int, H: int, p: float) -> np.ndarray:
    """[rows, H] bool: True where element (i, h) of layer ``l``'s type-``t`` output survives the step ``ctr``."""
    q = np.arange(rows * H, dtype=np.uint64).reshape(rows, H)
    return (raw_hash(seed, ctr, l, t, q) >> np.uint64(32)) >= np.uint64(drop_threshold(p))
