"""Exact three-plane oracles for the fp32 split-mode GEMMs (csrc/hgin_common.h: a = a1 + a2 + a3 in bf16 planes, a
product = the six MFMA terms a3b1, a2b2, a1b3, a2b1, a1b2, a1b1).  Plain torch, no kernel of the project: the host
test (tests/test_split_planes_host.py) runs it on the CPU, the GPU child (tests/split_child.py) with device="cuda".

A plane cannot be exercised alone (the planes are cut from one significand), so the operands are built such that the
mathematical result is exactly representable in fp32 while every minor term contributes to it: the kernel must then
return the float64 reference bit for bit, in any product or summation order.

Value classes (the components of one value share one random sign, so no rounding crosses a binade):
  T3  s (h + m 2^-10 + l 2^-19), h in {1,2,3}, m in {2,3}, l in {1,2,3}: host_split gives exactly (s h, s m 2^-10,
      s l 2^-19): three busy planes, nothing left after the third.
  T2  s (h + m 2^-10), h, m in {1,2,3}: plane 2 busy everywhere, plane 3 zero.
  T1  +-1, +-2: one plane.

Operands are dense tensors or Sparse selectors (a few nonzeros per row / a few live rows), so an output is one product
(or a handful) and every element of the dense operand reaches a checked output once the selector has as many rows as
the dense operand has columns.

Oracles (a = planes of the first operand A / g_z, b = planes of the second, W / B):
  O1   A dense T3, W selector T1      isolates a2b1, a3b1
  O2   A selector T1, W dense T3      isolates a1b2, a1b3
  O3   A dense T2, W selector T2      isolates a2b2 (and a2b1, a1b2)
  O3m  A selector T2, W dense T2      the mirror
  D1   A dense T2, W dense T1         a2b1 through the whole K loop of every accumulator (NT only)
  D1m  A dense T1, W dense T2         a1b2, the mirror (NT only)

nt_case / tn_case build a case and assert, on the reference alone: it round-trips through fp32; the planes have the
designed occupancy; sum |a||b| + |bias| + |accum| stays below 2^24 quanta of the output's grid at every stage of the
epilogue (so every partial sum is exact in every order); the six-term emulation equals the reference; dropping each
term the oracle isolates changes >= 99 % of the outputs (conditions(); the dense D1 / D1m: DENSE_FLOOR).  A case
carries its mutation table row: the share of outputs each dropped minor term changes."""
from dataclasses import dataclass

import torch

F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
TERMS = {"a3b1": (2, 0), "a2b2": (1, 1), "a1b3": (0, 2), "a2b1": (1, 0), "a1b2": (0, 1), "a1b1": (0, 0)}
MINOR = ("a3b1", "a2b2", "a1b3", "a2b1", "a1b2")
ISOLATES = {"O1": ("a2b1", "a3b1"), "O2": ("a1b2", "a1b3"), "O3": ("a2b2", "a2b1", "a1b2"),
            "O3m": ("a2b2", "a2b1", "a1b2"), "D1": ("a2b1",), "D1m": ("a1b2",)}
SELECTOR_ORACLES = ("O1", "O2", "O3", "O3m")
NT_ORACLES = SELECTOR_ORACLES + ("D1", "D1m")
TN_ORACLES = SELECTOR_ORACLES
Q10, Q19 = 2.0 ** -10, 2.0 ** -19
# the grid of a product of the two operand classes of an oracle
GRID = {"O1": Q19, "O2": Q19, "O3": Q10 * Q10, "O3m": Q10 * Q10, "D1": Q10, "D1m": Q10}
VMAX = {"T1": 2.0, "T2": 3.0 + 3 * Q10, "T3": 3.0 + 3 * Q10 + 3 * Q19}
CLASSES = {"O1": ("T3", "T1"), "O2": ("T1", "T3"), "O3": ("T2", "T2"), "O3m": ("T2", "T2"), "D1": ("T2", "T1"),
           "D1m": ("T1", "T2")}
# D1 / D1m: a dropped term changes an output unless sum_k m_k w_k = 0, a sum of K independent integers of variance
# E[m^2] E[w^2] = (14 / 3) (5 / 2) each: by the local limit theorem P(0) <= 2 / (sigma sqrt(2 pi)) < 0.03 at K >= 64
DENSE_FLOOR = 0.95
EMU_ROWS = 1024      # conditions(): the emulation and the mutations run on this many leading rows / live rows


def host_split(x):
    """The kernels' split2 restated: bf16 RNE, residuals in fp32.  x fp32 -> the three planes as fp32."""
    assert x.dtype == F32
    p1 = x.to(BF).float()
    r = x - p1
    p2 = r.to(BF).float()
    s = r - p2
    return p1, p2, s.to(BF).float()


def _ri(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g, device=g.device).float()


def values(cls, shape, g):
    """fp32 values of a class, drawn on the CPU generator g."""
    s = 2.0 * _ri(g, 0, 1, shape) - 1.0
    if cls == "T1":
        return s * _ri(g, 1, 2, shape)
    if cls == "T2":
        return s * (_ri(g, 1, 3, shape) + _ri(g, 1, 3, shape) * Q10)
    assert cls == "T3"
    return s * (_ri(g, 1, 3, shape) + _ri(g, 2, 3, shape) * Q10 + _ri(g, 1, 3, shape) * Q19)


@dataclass
class Sparse:
    """A [rows, width] fp32 operand given by its nonzeros (r, c, v)."""
    rows: int
    width: int
    r: torch.Tensor
    c: torch.Tensor
    v: torch.Tensor

    def dense(self):
        out = torch.zeros(self.rows, self.width, device=self.v.device)
        out[self.r, self.c] = self.v
        return out

    def first_rows(self, n):
        k = self.r < n
        return Sparse(n, self.width, self.r[k], self.c[k], self.v[k])

    def with_values(self, v):
        return Sparse(self.rows, self.width, self.r, self.c, v)


def _stride(width):
    """The selector's column step, coprime to the width (5; 7 where 5 divides the width)."""
    step = 5 if width % 5 else 7
    assert width % step != 0 or width == 1
    return step


def selector(rows, width, cls, g, off=0):
    """One nonzero per row: row r holds one value of the class at column (5 r + 3 + off) mod width (step 7 where 5
    divides the width).  With the step coprime to the width, `width` consecutive rows reach every column."""
    r = torch.arange(rows, device=g.device)
    return Sparse(rows, width, r, (_stride(width) * r + 3 + off) % width, values(cls, (rows,), g))


def row_selector(rows, width, block, every, cls, g):
    """The reduction's selector: one live row per `every` blocks of `block` rows, its place in the block rotating, one
    value of the class in it, at column (5 i + 3) mod width for the i-th live row."""
    nblk = -(-rows // block)
    b = torch.arange(0, nblk, every, device=g.device)
    i = torch.arange(b.numel(), device=g.device)
    r = b * block + i % block
    keep = r < rows
    r, i = r[keep], i[keep]
    return Sparse(rows, width, r, (_stride(width) * i + 3) % width, values(cls, (r.numel(),), g))


def planes(x):
    if isinstance(x, Sparse):
        return tuple(x.with_values(p) for p in host_split(x.v))
    return host_split(x)


def as_dense(x):
    return x.dense() if isinstance(x, Sparse) else x


def head(x, n):
    return x.first_rows(n) if isinstance(x, Sparse) else x[:n]


def _abs(x):
    return x.with_values(x.v.abs()) if isinstance(x, Sparse) else x.abs()


def mm_nt(a, w):
    """float64 a [M, K] @ w[N, K]^T of dense / Sparse operands."""
    if isinstance(w, Sparse):
        out = torch.zeros(a.shape[0], w.rows, dtype=F64, device=a.device)
        return out.index_add_(1, w.r, a.double()[:, w.c] * w.v.double())
    if isinstance(a, Sparse):
        out = torch.zeros(a.rows, w.shape[0], dtype=F64, device=w.device)
        return out.index_add_(0, a.r, a.v.double()[:, None] * w.double().t()[a.c])
    return a.double() @ w.double().t()


def mm_tn(a, b):
    """float64 a[M, N]^T @ b [M, K] of dense / Sparse operands."""
    if isinstance(a, Sparse):
        out = torch.zeros(a.width, b.shape[1], dtype=F64, device=b.device)
        return out.index_add_(0, a.c, a.v.double()[:, None] * b.double()[a.r])
    if isinstance(b, Sparse):
        out = torch.zeros(b.width, a.shape[1], dtype=F64, device=a.device)
        return out.index_add_(0, b.c, b.v.double()[:, None] * a.double()[b.r]).t().contiguous()
    return a.double().t() @ b.double()


def six_terms(mm, a, b, drop=()):
    """The split product restated: the sum of the six plane products (all but `drop`), each formed exactly."""
    pa, pb = planes(a), planes(b)
    out = None
    for name, (i, j) in TERMS.items():
        if name not in drop:
            t = mm(pa[i], pb[j])
            out = t if out is None else out + t
    return out


def occupancy(x, cls):
    """The designed plane occupancy of a class on the nonzeros of x."""
    v = x.v if isinstance(x, Sparse) else x
    p1, p2, p3 = host_split(v)
    assert torch.equal(p1.double() + p2.double() + p3.double(), v.double()), "residual after plane 3"
    assert bool((p1 != 0).all())
    if cls == "T1":
        assert bool((p2 == 0).all()) and bool((p3 == 0).all())
    elif cls == "T2":
        assert bool((p2 != 0).all()) and bool((p3 == 0).all())
    else:
        assert bool((p2 != 0).all()) and bool((p3 != 0).all())


def exact_in_fp32(ref, mag, q, what=""):
    """ref (float64) lies on the grid q (a number, or a tensor broadcast over the outputs), round-trips through fp32,
    and mag = the sum of the magnitudes of everything added into it stays below 2^24 q: every partial sum, in any order,
    is then a multiple of q below 2^24 q, so exact in fp32."""
    q = torch.as_tensor(q, dtype=F64, device=ref.device)
    assert torch.equal(ref, torch.round(ref / q) * q), (what, "off the grid")
    assert torch.equal(ref, ref.float().double()), (what, "does not round-trip through fp32")
    assert bool((mag < 2.0 ** 24 * q).all()), (what, float((mag / q).max()))


def conditions(oracle, mm, a, b, acc, rows_a=True, floor=0.99):
    """The emulation and mutation conditions of one case on its product acc = mm(a, b) (float64), restricted to the
    first EMU_ROWS rows (NT: output rows; TN: the rows of the reduction) when the operands are larger: rows are
    drawn alike.  Returns {minor term: share of outputs changed}."""
    if rows_a:                                    # NT: operand a's rows are the output's
        n = min(EMU_ROWS, acc.shape[0])
        a, want = head(a, n), acc[:n]
    else:                                         # TN: both operands share the reduced rows
        n = a.rows if isinstance(a, Sparse) else a.shape[0]
        if n > 4 * EMU_ROWS:
            n = 4 * EMU_ROWS
            a, b = head(a, n), head(b, n)
            want = mm(a, b)
        else:
            want = acc
    assert torch.equal(six_terms(mm, a, b), want), (oracle, "six-term emulation != reference")
    live = want != 0 if not rows_a else torch.ones_like(want, dtype=torch.bool)
    table = {}
    for term in MINOR:
        got = six_terms(mm, a, b, drop=(term,))
        table[term] = float(((got != want) & live).sum()) / max(1, int(live.sum()))
    for term in ISOLATES[oracle]:
        assert table[term] >= (DENSE_FLOOR if oracle in ("D1", "D1m") else floor), (oracle, term, table[term])
    return table



# ----------------------------------------------------------------------------------------------------------------------
# cases: operands, epilogue operands, the float64 reference of every output, the conditions, the mutation table row
# ----------------------------------------------------------------------------------------------------------------------
SLOPE = 0.5          # PReLU slope: a power of two, so the negative branch is exact
SCALE = 2.0          # 1 + eps of the self term (eps = 1.0)


def prelu(z, slope):
    return torch.where(z > 0, z, slope * z)


def _scaled(x, k1, K):
    """[x[:, :k1] | SCALE x[:, k1:]]: the two-source A as the kernels form it."""
    if k1 in (0, K):
        return x
    if isinstance(x, Sparse):
        return x.with_values(torch.where(x.c >= k1, SCALE * x.v, x.v))
    out = x.clone()
    out[:, k1:] *= SCALE
    return out


def nt_case(oracle, kind, M, N, K, seed, k1=0, accum=False, prev=False, off=0, device="cpu"):
    """An NT case.  kind: "fwd" (y = prelu(A W^T + b) [+ accum], z kept), "lin" (y = A W^T + b), "plain" (c = A W^T),
    "comb" (c, g_x_dst = SCALE c [+ g_prev], g_eps = sum c x_dst).  k1: the columns of the first of two A sources,
    the second one scaled by SCALE in the kernel's loads (fwd only).  Returns {"in": fp32 tensors, "ref": float64
    outputs, "table": mutation row, "xd": ...}."""
    g = torch.Generator(device=device).manual_seed(seed)
    ca, cw = CLASSES[oracle]
    if oracle in ("O1", "O3"):
        a, w = values(ca, (M, K), g), selector(N, K, cw, g, off)
    elif oracle in ("O2", "O3m"):
        a, w = selector(M, K, ca, g, off), values(cw, (N, K), g)
    else:
        a, w = values(ca, (M, K), g), values(cw, (N, K), g)
    ae = _scaled(a, k1, K)
    occupancy(ae, ca)
    occupancy(w, cw)
    acc, mag = mm_nt(ae, w), mm_nt(_abs(ae), _abs(w))
    # the grid of an output: a selector's single product lies on SCALE q where it reads the scaled columns
    q = torch.tensor(GRID[oracle], dtype=F64, device=device)
    if k1 not in (0, K) and isinstance(w, Sparse):
        q = q * torch.where(w.c >= k1, SCALE, 1.0).double()[None, :]
    elif k1 not in (0, K) and isinstance(a, Sparse):
        q = q * torch.where(a.c >= k1, SCALE, 1.0).double()[:, None]
    exact_in_fp32(acc, mag, q, (oracle, kind, "acc"))
    ri = lambda lo, hi, *s: _ri(g, lo, hi, s)   # noqa: E731
    dense_a = as_dense(a)
    ins = {"w": as_dense(w)}
    if k1 not in (0, K):
        ins["a1"], ins["a2"] = dense_a[:, :k1].contiguous(), dense_a[:, k1:].contiguous()
    else:
        ins["a1"] = dense_a
    ref = {}
    if kind in ("fwd", "lin"):
        ins["b"] = ri(-1, 1, N)
        z, magz = acc + ins["b"].double(), mag + ins["b"].double().abs()
        exact_in_fp32(z, magz, q, (oracle, kind, "z"))
        if kind == "lin":
            ref["y"] = z
        else:
            y, magy = prelu(z, SLOPE), SLOPE * magz
            if accum:
                ins["accum"] = ri(-2, 2, M, N)
                y, magy = y + ins["accum"].double(), magy + ins["accum"].double().abs()
            exact_in_fp32(y, magy, SLOPE * q, (oracle, kind, "y"))
            ref["z"], ref["y"] = z, y
    elif kind == "plain":
        ref["c"] = acc
    else:
        assert kind == "comb"
        ins["xd"] = ri(-2, 2, M, N)
        gx, maggx = SCALE * acc, SCALE * mag
        if prev:
            ins["prev"] = ri(-2, 2, M, N)
            gx, maggx = gx + ins["prev"].double(), maggx + ins["prev"].double().abs()
        exact_in_fp32(gx, maggx, SCALE * q, (oracle, kind, "gx"))     # SCALE c and the integers: the grid SCALE q
        ref["c"], ref["gx"] = acc, gx
    table = conditions(oracle, mm_nt, ae, w, acc)
    return {"in": ins, "ref": ref, "table": table}


def tn_every(oracle, M, width, cap):
    """Blocks of 16 rows between live rows of the TN selector: the fewest such that the live rows that share an output
    keep sum |a||b| below `cap`; one row per output where a single product already exceeds it (a lone product needs
    only to be representable, which exact_in_fp32 asserts on the reference)."""
    ca, cb = CLASSES[oracle]
    per_max = max(1, int(cap / (VMAX[ca] * VMAX[cb])))
    nblk = -(-M // 16)
    every = 1
    while -(-(-(-nblk // every)) // width) > per_max:
        every += 1
    return every


def tn_case(oracle, M, N, K, seed, fused, device="cpu"):
    """A TN case: out[N, K] = A^T B reduced over the M rows, A = g_y (plain) or g_z = where(z > 0, g_y, SLOPE g_y)
    formed by the kernel (fused; z random with exact zeros).  Returns {"in": {gy, z, b}, "ref": {g_w, g_z, g_b, g_a},
    "table"}; g_b / g_a are float64 sums for the tolerance checks."""
    g = torch.Generator(device=device).manual_seed(seed)
    ca, cb = CLASSES[oracle]
    q = GRID[oracle] * (SLOPE if fused else 1.0)
    cap = 2.0 ** 24 * q
    if oracle in ("O2", "O3m"):
        gy = row_selector(M, N, 16, tn_every(oracle, M, N, cap), ca, g)
        b = values(cb, (M, K), g)
    else:
        gy = values(ca, (M, N), g)
        b = row_selector(M, K, 16, tn_every(oracle, M, K, cap), cb, g)
    # the products that meet in one output share a sign (live row m of the dense operand: the selector value's sign
    # times a random sign per column), so the part a dropped term takes out of an output cannot cancel over its rows
    sel, dense = (gy, b) if isinstance(gy, Sparse) else (b, gy)
    colsign = 2.0 * _ri(g, 0, 1, (dense.shape[1],)) - 1.0
    dense[sel.r] = dense[sel.r].abs() * torch.sign(sel.v)[:, None] * colsign[None, :]
    occupancy(gy, ca)
    occupancy(b, cb)
    ins = {"gy": as_dense(gy), "b": as_dense(b)}
    gz = gy
    if fused:
        z = torch.randn(M, N, generator=g, device=device)
        z[torch.rand(M, N, generator=g, device=device) < 0.125] = 0.0
        ins["z"] = z
        if isinstance(gy, Sparse):
            gz = gy.with_values(torch.where(z[gy.r, gy.c] > 0, gy.v, SLOPE * gy.v))
        else:
            gz = torch.where(z > 0, gy, SLOPE * gy)
        occupancy(gz, ca)
    acc, mag = mm_tn(gz, b), mm_tn(_abs(gz), _abs(b))
    ones = lambda x: x.with_values(torch.ones_like(x.v)) if isinstance(x, Sparse) else torch.ones_like(x)   # noqa: E731
    cnt = mm_tn(ones(gz), ones(b)) if isinstance(gz, Sparse) or isinstance(b, Sparse) else None
    assert cnt is not None
    # an output of several products: all on the grid q, below 2^24 q.  A lone product (an unhalved one lies on the
    # grid q / SLOPE): representable is enough, every partial sum of its six terms is a subset sum below it
    lone = cnt <= 1
    exact_in_fp32(torch.where(lone, 0.0, acc), torch.where(lone, 0.0, mag), q, (oracle, "g_w"))
    assert torch.equal(acc, acc.float().double()) and bool((mag < 2.0 ** 24 * q / SLOPE).all()), (oracle, "g_w lone")
    gzd = as_dense(gz).double()
    ref = {"g_w": acc, "g_z": gzd, "g_b": gzd.sum(0), "g_b_mag": gzd.abs().sum(0)}
    if fused:
        zr, gyd = ins["z"].double(), ins["gy"].double()
        ref["g_a"] = (torch.where(zr > 0, torch.zeros_like(zr), zr) * gyd).sum()
        ref["g_a_mag"] = (zr * gyd).abs().sum()
    table = conditions(oracle, mm_tn, gz, b, acc, rows_a=False)
    return {"in": ins, "ref": ref, "table": table}
