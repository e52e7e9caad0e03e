"""Inputs and float64 references of the exact contrastive-head tests.  Nothing here touches a device: the generators
and references are themselves checked by tests/test_head_cases_cpu.py.

Exactness: GEMM operands are integers in [-3, 3] (every partial sum below 2^24, any association exact); feature vectors
have n = 4^j non-zero entries of +-1 / sqrt(n), so norms and dot products (multiples of 1/n) are exact and similarities
tie often; logits of the loss live on a grid of 1/4."""
import math

import torch

NEG_INF = -float("inf")


def gen(*key):
    """A generator seeded by the integers of `key` (the shape of a row, mostly): every row has its own data."""
    g = torch.Generator()
    seed = 12345
    for k in key:
        seed = (seed * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    g.manual_seed(seed)
    return g


def is_fp32(t):
    """Every value of the float64 tensor is an fp32 value."""
    return bool((t.float().double() == t).all())


def ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


# ---- feature vectors ---------------------------------------------------------------------------------------------------

def unit_rows(n, D, nnz, g):
    """(n, D) float64: `nnz` entries of +-1/sqrt(nnz) per row (nnz a power of 4), the rest 0."""
    out = torch.zeros(n, D, dtype=torch.float64)
    v = 1.0 / math.sqrt(nnz)
    for r in range(n):
        where = torch.randperm(D, generator=g)[:nnz]
        out[r, where] = (torch.randint(0, 2, (nnz,), generator=g).double() * 2 - 1) * v
    return out


def nnz_for(D):
    return 64 if D >= 128 else 16 if D >= 16 else 1


def tie_columns(ties, K):
    return sorted({c % K for c in ties if -K <= c < K})


def head_features(B, K, D, g, ties=()):
    """q, k (B, D) and queue (D, K): unit vectors as above.  The columns named by `ties` all hold one vector h, which is
    also feature row 0 and every third one after it: for those rows the tied columns are the row maximum (similarity 1);
    for every other row they tie at some lower value."""
    nnz = nnz_for(D)
    q = unit_rows(B, D, nnz, g)
    k = unit_rows(B, D, nnz, g)
    queue = unit_rows(K, D, nnz, g).t().contiguous()
    cols = tie_columns(ties, K)
    if cols:
        h = unit_rows(1, D, nnz, g)[0]
        queue[:, cols] = h[:, None]
        q[0::3] = h
    return q, k, queue


def inv_T_of(T):
    """1.f / T as the library forms it (fp32 division of the fp32 argument)."""
    return float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(T, dtype=torch.float32))


def logits_reference(q, k, queue, T):
    """float64 logits with ONE rounding: fp32(similarity * inv_T), the similarity being exact."""
    s = torch.cat([(q * k).sum(1, keepdim=True), q @ queue], 1)
    return (s * inv_T_of(T)).float().double(), s


# ---- ordered top-k -----------------------------------------------------------------------------------------------------

def ordered_topk(s, k):
    """Columns of the k first elements of every row in (value descending, column ascending) order: repeated selection
    with ties to the lowest column, -inf entries last, lowest column first."""
    return torch.sort(s, dim=1, descending=True, stable=True).indices[:, :k]


def mask_reference(sim, src, names, topk):
    """(B, 1 + K) uint8: column 0, the same-source columns, and the ordered top-k of the other columns."""
    same = src[:, None] == names[None, :]
    m = same.clone()
    if topk > 0:
        idx = ordered_topk(sim.masked_fill(same, NEG_INF), topk)
        m.scatter_(1, idx, True)
    return torch.cat([torch.ones(len(src), 1, dtype=torch.bool), m], 1).to(torch.uint8)


def names_variant(variant, B, K, g):
    """(src (B,), names (K,)) int64.  mixed: four sources and -1 entries on both sides; sparse: every column but three
    is source 9 (rows of source 9 have 3 non-sibling columns); full: every column is source 9 (they have none)."""
    if variant == "mixed":
        src = torch.randint(0, 4, (B,), generator=g)
        names = torch.randint(0, 4, (K,), generator=g)
        names[torch.randperm(K, generator=g)[:max(1, K // 9)]] = -1
        if B > 2:
            src[2] = -1
        return src, names
    src = torch.where(torch.arange(B) % 2 == 0, 9, 2)
    names = torch.full((K,), 9, dtype=torch.int64)
    if variant == "sparse":
        free = torch.randperm(K, generator=g)[:3]
        names[free] = torch.tensor([-1, 2, 5])[:len(free)]
    return src, names


def retrieval_inputs(B, N, ks, g):
    """sim (B, N) on a grid of 1/64 with few distinct values (ties across every pick boundary), labels such that row 0's
    only match sits exactly at rank k* and row 1's exactly at rank k* + 1 (k* the middle entry of ks); the other rows
    draw their labels from a small set."""
    sim = ints((B, N), -6, 6, g) / 64.0
    kmax = ks[-1]
    order = ordered_topk(sim, min(N, kmax + 1))
    train = torch.randint(0, 5, (N,), generator=g)
    test = torch.randint(0, 5, (B,), generator=g)
    kstar = ks[len(ks) // 2]
    pins = [(0, kstar - 1)] + ([(1, kstar)] if B > 1 and kstar < order.shape[1] else [])
    used = set()
    for b, rank in pins:
        col = int(order[b, rank])
        assert col not in used
        used.add(col)
        test[b] = 100 + b
        train[col] = 100 + b
    return sim, train, test


def retrieval_reference(sim, train, test, ks):
    idx = ordered_topk(sim, ks[-1])
    match = train[idx] == test[:, None]
    hits = torch.stack([match[:, :k].any(1) for k in ks], 1).float()
    return hits, idx.to(torch.int32)


# ---- loss --------------------------------------------------------------------------------------------------------------

LARGE = 320.0        # rows scaled to +-960: exp(v - max) underflows for most of the row


def loss_inputs(mode, drop_self, B, N1, g):
    """logits (B, N1) float64 on a grid of 1/4 in [-3, 3]; rows b % 7 == 1 scaled by LARGE, rows b % 7 == 5 constant.
    positives (B, N1) bool: mode 0 the one-hot of a target that visits column 0, the last column and a column >= 256;
    modes 1 / 2 a mask whose rows cycle through: column 0 + a few, only the last column, exactly one positive (column
    0), several with column 0, several without column 0 (mask[b][0] == 0).  Every row has a positive."""
    lg = ints((B, N1), -12, 12, g) / 4.0
    for b in range(B):
        if b % 7 == 1:
            lg[b] *= LARGE
        if b % 7 == 5:
            lg[b] = 1.5
    pos = torch.zeros(B, N1, dtype=torch.bool)
    target = None
    if mode == 0:
        target = torch.randint(0, N1, (B,), generator=g)
        special = [0, N1 - 1, min(N1 - 1, 256 + 3), N1 // 2]
        for b in range(B):
            if b % 3 != 2:
                target[b] = special[(b // 3 + b) % 4]
        pos[torch.arange(B), target] = True
    else:
        for b in range(B):
            kind = b % 5
            few = torch.randperm(N1, generator=g)[:min(N1, 4)]
            if kind == 0:
                pos[b, few] = True
                pos[b, 0] = True
            elif kind == 1:
                pos[b, N1 - 1] = True
            elif kind == 2:
                pos[b, 0] = True
            elif kind == 3:
                pos[b, few] = True
                pos[b, 0] = True
                pos[b, N1 - 1] = True
            else:
                pos[b, few] = True
                pos[b, 0] = False
                if not bool(pos[b].any()):
                    pos[b, N1 - 1] = True
    return lg, pos, target


def loss_reference(lg, pos, mode, drop_self, k1=1, k2=5):
    """float64 row statistics of coclr_amd/csrc/loss.hip: dict of loss, lse, aux (B,), hits (B, 4) by the rank rule
    (fewer than k logits strictly greater than the best positive / than column 0), drop (B,) and the five scalars.
    `lg` may require grad."""
    B = lg.shape[0]
    det = lg.detach()
    drop = torch.zeros(B, dtype=torch.bool)
    if mode == 1 and drop_self:
        drop = (pos.sum(1) != 1) & pos[:, 0]
    eff = pos.clone()
    eff[drop, 0] = False
    lse = torch.logsumexp(lg, 1)
    if mode == 2:
        n = eff.sum(1).double()
        loss = lse - torch.where(eff, lg, torch.zeros_like(lg)).sum(1) / n
        aux = n
    else:
        aux = torch.logsumexp(torch.where(eff, lg, torch.full_like(lg, NEG_INF)), 1)
        loss = lse - aux
    pmax = torch.where(pos, det, torch.full_like(det, NEG_INF)).max(1).values
    cgp = (det > pmax[:, None]).sum(1)
    cg0 = (det > det[:, :1]).sum(1)
    hits = torch.stack([cgp < k1, cgp < k2, cg0 < k1, cg0 < k2], 1).double()
    scalars = torch.cat([loss.detach().mean(0, keepdim=True), hits.mean(0)])
    return dict(loss=loss, lse=lse, aux=aux, hits=hits, drop=drop, scalars=scalars, eff=eff)


def loss_gradient(lg, pos, mode, drop_self, dloss):
    """d(dloss * mean loss) / d logits by float64 autograd."""
    x = lg.clone().requires_grad_(True)
    r = loss_reference(x, pos, mode, drop_self)
    (r["loss"].mean() * dloss).backward()
    return x.grad


def tie_free(lg):
    """Rows of the matrix without two equal entries."""
    s = torch.sort(lg, dim=1).values
    return (s[:, 1:] != s[:, :-1]).all(1) if lg.shape[1] > 1 else torch.ones(lg.shape[0], dtype=torch.bool)


# ---- launcher predicates (mirrors of the host code) --------------------------------------------------------------------

def cdiv(a, b):
    return (a + b - 1) // b


def gemm_branch(M, N, K, sam, sak, sbk, sbn, splits, mode=0, fused=False):
    """What launch_gemm of nce.hip decides: layout, slice, effective splits, direct / folded, fold kernel, RC."""
    kslice = cdiv(cdiv(K, splits), 32) * 32
    eff = cdiv(K, kslice)
    to_part = eff > 1 or (fused and not (mode == 0 and splits == 1))
    fold = None
    if to_part:
        fold = "rows" if mode in (2, 3) else "expand" if mode == 4 else "plain"
    return dict(TA=(sam == 1 and sak != 1), TB=(sbk == 1 and sbn != 1), kslice=kslice, splits=eff,
                partial_last=K % kslice != 0, folded=to_part, fold=fold,
                RC=(2 if N <= 128 else 8) if fold == "rows" else None,
                grid=(cdiv(N, 128), cdiv(M, 32), eff))


def operand_strides(rows, cols, pad, transposed):
    """(stride of the row index, stride of the column index) of a tests/_exact.source2d operand."""
    return (1, rows + pad) if transposed else (cols + pad, 1)


def logits_branch(D, q_shift):
    return "fused" if D == 128 and (4 * q_shift) % 16 == 0 else "fallback"


def copy_branch(row_elems, in_row_stride, shift_in, shift_out):
    vec = (row_elems | in_row_stride) % 4 == 0 and (4 * shift_in) % 16 == 0 and (4 * shift_out) % 16 == 0
    gx = min(256, max(1, (row_elems // 4 + 255) // 256))
    per_pass = gx * 256 * (4 if vec else 1)
    return dict(vector=vec, gx=gx, loops=row_elems > per_pass)


def pull_branch(row_elems, shift_in):
    return copy_branch(row_elems, row_elems if row_elems % 4 == 0 else 1, shift_in, 0)


def retrieval_use_lds(N):
    return 4 * N <= 150 * 1024


def mask_lds_ok(K, topk):
    return (4 * K if topk > 0 else 0) <= 150 * 1024
