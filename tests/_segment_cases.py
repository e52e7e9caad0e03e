"""Case table, host predicates and float64 references of the exact tests of the two segmented-accumulate kernels
(coclr_amd/csrc/retrieval.hip: coclr_segment_softmax_accum, coclr_segment_accum), plain data and CPU torch only.

  out[o][:] += w * sum_{r ascending} f(x[first + r][:]),    f = softmax over the row, or the identity

A row of the table is one call: widths, operand alignment, the segments (first row, rows, output row) in list order, their
weights and the class of its data.  `branches(row)` restates what the launcher decides on the host (16-byte or scalar
form and why, passes and tail of the column loop, idle waves, which segments share a launch);
tests/test_segment_cases_cpu.py asserts that the rows reach every such branch and pins the restatement to the library,
tests/test_gpu_segment_exact.py holds the kernels to the references.

Data classes:
  sum      small integers, power-of-two weights (0 and negative ones among them), a prior in units of the smallest weight:
           every partial sum is an integer below 2^10 and the result is determined bit for bit (segment_accum)
  softmax  in every row k in {1, 2, 4, 8} columns hold the row's maximum v and all others v - 200 or less, -inf among
           them: expf gives exactly 1 and exactly 0, the denominator is exactly k, the probabilities exactly 1/k and 0
           (segment_softmax_accum).  The maximal columns of row r all belong to ONE wave of ONE pass of the column loop,
           which rotates with r over the four waves, the first, second and last pass, and the last column.
  rand3, rand30   randn * 3 / * 30, weights 1 / rows, a randn prior (both kernels, 1e-6 of the largest reference element)
"""
import collections
import functools
import zlib

import torch

SEG_MAX = 64            # COCLR_SEG_MAX: segments per launch
MAX_C = 4096            # COCLR_SEG_MAX_C
THREADS = 256
WAVE = 64
INF = float("inf")

EXACT = ("sum", "softmax")
RANDOM = ("rand3", "rand30")
SMALLEST_WEIGHT = 2.0 ** -6

Seg = collections.namedtuple("Seg", "name C x_shift out_shift R V segs weights cls group")


# ---- the launcher's host predicates (retrieval.hip, segment_accum<>) ----------------------------------------------------

def accepted(R, C, S, V, segs):
    """The validation that precedes every launch."""
    if R <= 0 or S <= 0 or V <= 0 or C < 1 or C > MAX_C:
        return False
    return all(first >= 0 and rows >= 1 and first + rows <= R and 0 <= o < V for first, rows, o in segs)


def partition(outs):
    """[(segment indices of one launch, why the launch was cut: a subset of {"full", "same row"}, or {"end"})]."""
    blocks, cur = [], []
    for s, o in enumerate(outs):
        why = set()
        if len(cur) == SEG_MAX:
            why.add("full")
        if any(outs[j] == o for j in cur):
            why.add("same row")
        if why and cur:
            blocks.append((cur, why))
            cur = []
        cur.append(s)
    blocks.append((cur, {"end"}))
    return blocks


def branches(row):
    scalar_why = set()
    if row.C % 4:
        scalar_why.add("C % 4")
    if row.x_shift % 4:
        scalar_why.add("x base")
    if row.out_shift % 4:
        scalar_why.add("out base")
    vec = not scalar_why
    cv = row.C // (4 if vec else 1)                  # columns in units of the thread's load
    blocks = partition([o for _, _, o in row.segs])
    return {"vec": vec, "scalar_why": scalar_why, "VEC": 4 if vec else 1, "CV": cv,
            "passes": -(-cv // THREADS), "tail": cv % THREADS, "idle_waves": max(0, 4 - -(-cv // WAVE)),
            "launches": [b for b, _ in blocks], "cuts": [why for _, why in blocks[:-1]],
            "lds_bytes": 2 * row.C * 4}


def owner(row, column):
    """(pass, wave) of the thread that owns `column` in the form the row runs in."""
    unit = column // branches(row)["VEC"]
    return unit // THREADS, unit % THREADS // WAVE


def slots(row):
    """The (pass, wave) pairs the maximal columns rotate over: every wave that has a column, in the first, the second
    and the last pass."""
    b = branches(row)
    out = []
    for p in sorted({0, min(1, b["passes"] - 1), b["passes"] - 1}):
        for w in range(4):
            if p * THREADS + w * WAVE < b["CV"]:
                out.append((p, w))
    return out


def max_columns(row, r):
    """The columns of x row r that hold the row's maximum: all owned by slot r mod (slots + 1); the extra turn is the
    last column alone."""
    b = branches(row)
    sl = slots(row)
    turn = r % (len(sl) + 1)
    if turn == len(sl):
        return [row.C - 1]
    p, w = sl[turn]
    u0 = p * THREADS + w * WAVE
    c0, c1 = u0 * b["VEC"], min(u0 + WAVE, b["CV"]) * b["VEC"]
    want = (1, 2, 4, 8)[(turn + r // (len(sl) + 1)) % 4]
    k = max(kk for kk in (1, 2, 4, 8) if kk <= min(want, c1 - c0))
    start = c0 + (7 * r) % (c1 - c0 - k + 1)
    stride = (c1 - 1 - start) // (k - 1) if k > 1 and r % 2 == 0 else 1      # spread over the slot, or adjacent
    return [start + i * stride for i in range(k)]


# ---- data -----------------------------------------------------------------------------------------------------------------

ROW_MAXIMA = (87.0, -1000.0, 3.0e4, 0.0, -3.5, 12.25)


def gen(row):
    """Seeded by the call's shape and class, NOT by its name or alignment: the twins of a row hold the same data."""
    key = repr((row.C, row.R, row.V, tuple(row.segs), row.cls)).encode()
    return torch.Generator().manual_seed(zlib.crc32(key))


@functools.lru_cache(maxsize=None)
def inputs(row):
    """(x (R, C), prior (V, C)) as fp32 values in float64 tensors.  Do not write to them: they are shared."""
    g = gen(row)
    R, C, V = row.R, row.C, row.V
    if row.cls == "sum":
        x = torch.randint(-8, 9, (R, C), generator=g).double()
        prior = torch.randint(-32, 33, (V, C), generator=g).double() * SMALLEST_WEIGHT
    elif row.cls == "softmax":
        x = torch.empty(R, C, dtype=torch.float64)
        low = torch.randint(0, 10, (R, C), generator=g)
        for r in range(R):
            v = ROW_MAXIMA[r % len(ROW_MAXIMA)]
            x[r] = v - 200.0 - 0.5 * low[r].double()              # steps 0 .. 7 below v - 200 ...
            x[r][low[r] >= 8] = -INF                               # ... and a fifth of the columns -inf
            x[r][max_columns(row, r)] = v
        prior = torch.randint(-32, 33, (V, C), generator=g).double() * SMALLEST_WEIGHT
    else:
        scale = {"rand3": 3.0, "rand30": 30.0}[row.cls]
        x = (torch.randn(R, C, generator=g) * scale).double()
        prior = torch.randn(V, C, generator=g).double()
    assert torch.equal(x.float().double(), x) and torch.equal(prior.float().double(), prior)
    return x, prior


def unread_rows(row):
    used = set()
    for first, rows, _ in row.segs:
        used.update(range(first, first + rows))
    return [r for r in range(row.R) if r not in used]


def unnamed_outputs(row):
    return sorted(set(range(row.V)) - {o for _, _, o in row.segs})


def plain_reference(row, softmax):
    """The per-video expression in float64, segments applied in list order."""
    x, prior = inputs(row)
    out = prior.clone()
    for (first, rows, o), w in zip(row.segs, row.weights):
        part = x[first:first + rows]
        part = torch.softmax(part, -1) if softmax else part
        out[o] += w * part.sum(0)
    return out


def exact_steps(row):
    """The table after every segment of an EXACT row, from the closed form of its class: integer sums for `sum`; for
    `softmax` 1/k in the row's maximal columns and 0 elsewhere, without an exponential."""
    assert row.cls in EXACT
    x, prior = inputs(row)
    out = prior.clone()
    for (first, rows, o), w in zip(row.segs, row.weights):
        if row.cls == "sum":
            acc = x[first:first + rows].sum(0)
        else:
            acc = torch.zeros(row.C, dtype=torch.float64)
            for r in range(first, first + rows):
                cols = max_columns(row, r)
                acc[cols] += 1.0 / len(cols)
        out[o] += w * acc
        yield out.clone()


@functools.lru_cache(maxsize=None)
def reference(row, softmax):
    """float64 (V, C).  Shared: do not write to it."""
    if row.cls in EXACT:
        assert softmax == (row.cls == "softmax")
        return list(exact_steps(row))[-1]
    return plain_reference(row, softmax)


def kernels_of(row):
    """Which of (softmax, plain) the row's class is data for."""
    return {"sum": (False,), "softmax": (True,)}.get(row.cls, (True, False))


def restated_fp32(row, softmax):
    """The operation in fp32 torch on the CPU: softmax in fp32, rows added in ascending order, times the weight."""
    x, prior = inputs(row)
    x, out = x.float(), prior.float().clone()
    for (first, rows, o), w in zip(row.segs, row.weights):
        acc = torch.zeros(row.C, dtype=torch.float32)
        for r in range(first, first + rows):
            acc += torch.nn.functional.softmax(x[r], -1) if softmax else x[r]
        out[o] += torch.tensor(w, dtype=torch.float32) * acc
    return out


# ---- the table ------------------------------------------------------------------------------------------------------------

def _pow2_weight(s, rows):
    """Exact rows: 1 / rows where that is a power of two, else a rotation that holds 0 and negative powers of two."""
    if rows & (rows - 1) == 0:
        return 1.0 / rows
    return (0.5, -0.25, 1.0, 0.0, SMALLEST_WEIGHT, -2.0)[s % 6]


def _rows(name, group, C, R, V, segs, x_shift=0, out_shift=0, weights=None, classes=EXACT + RANDOM):
    out = []
    for cls in classes:
        if cls in EXACT:
            w = weights if weights is not None else [_pow2_weight(s, rows) for s, (_, rows, _) in enumerate(segs)]
        else:
            w = [1.0 / rows for _, rows, _ in segs]
        out.append(Seg("%s-%s" % (name, cls), C, x_shift, out_shift, R, V, tuple(segs), tuple(w), cls, group))
    return out


# widths and bases: four segments over rows 1 .. 38 of 40 (38 consecutive rows: every slot of max_columns gets its turn),
# output rows 1, 3 and 5 of 7 named by nobody
WIDTH_SEGS = [(1, 13, 2), (14, 1, 0), (15, 16, 4), (31, 8, 6)]
WIDTH_WEIGHTS = [0.5, 1.0, 1.0 / 16, -0.25]
VEC_WIDTHS = (4, 252, 256, 1024, 1028, 2048, 4092, 4096)
SCALAR_WIDTHS = (1, 3, 63, 65, 255, 257, 513, 4093)
BASE_WIDTHS = (8, 1028)
BASE_SHIFTS = ((1, 0), (0, 2), (1, 2))               # (x_shift, out_shift)

# launch partition, as the output rows of consecutive segments
PARTITION_C = (12, 257)


def _distinct(n):
    return list(range(n))


PARTITIONS = (
    ("s64", _distinct(64)),                                            # one full launch
    ("s65", _distinct(65)),                                            # cut because the block is full
    ("s129", _distinct(129)),                                          # three launches
    ("dup-adjacent", [0, 1, 1, 2, 3, 4]),
    ("dup-ten-later", [o if o != 12 else 2 for o in range(14)]),
    ("triple", [0, 1, 0, 2, 0, 3]),                                    # three launches
    ("dup-as-65th", _distinct(64) + [5, 64]),                          # full AND the same row at once
    ("s1", [0]),
)

# geometry: the last row of x, the last row of out, nothing in row 0, out of row order, the same rows read twice, an
# output row nobody names (4), rows of x nobody reads, one row and 64 rows; weights 1 / rows, 0, negative
GEOMETRY_C = (12, 257)
GEOMETRY_SEGS = [(36, 64, 5), (20, 1, 0), (3, 9, 3), (3, 9, 1), (24, 4, 2)]
GEOMETRY_WEIGHTS = [1.0 / 64, 1.0, 0.0, -0.25, 0.25]


def _partition_segs(outs):
    segs, pos = [], 1                                # row 0 is read by nobody
    for s, o in enumerate(outs):
        rows = 1 + s % 2
        segs.append((pos, rows, o))
        pos += rows
    return segs, pos + 1, max(outs) + 3              # R: one unread row at the end too; V: two unnamed rows at the end


def _table():
    t = []
    for C in VEC_WIDTHS + SCALAR_WIDTHS:
        t += _rows("width-C%d" % C, "width", C, 40, 7, WIDTH_SEGS, weights=WIDTH_WEIGHTS)
    for C in BASE_WIDTHS:
        if C not in VEC_WIDTHS:
            t += _rows("base-C%d-aligned" % C, "base", C, 40, 7, WIDTH_SEGS, weights=WIDTH_WEIGHTS)
        for xs, os_ in BASE_SHIFTS:
            t += _rows("base-C%d-x%d-out%d" % (C, xs, os_), "base", C, 40, 7, WIDTH_SEGS, xs, os_, weights=WIDTH_WEIGHTS)
    for C in PARTITION_C:
        for name, outs in PARTITIONS:
            segs, R, V = _partition_segs(outs)
            t += _rows("part-C%d-%s" % (C, name), "partition", C, R, V, segs, classes=("sum", "softmax", "rand3"))
    for C in GEOMETRY_C:
        t += _rows("geometry-C%d" % C, "geometry", C, 100, 6, GEOMETRY_SEGS, weights=GEOMETRY_WEIGHTS)
    return t


CASES = _table()
BY_NAME = {c.name: c for c in CASES}


def of(group=None, cls=None):
    return [c for c in CASES if (group is None or c.group == group) and (cls is None or c.cls == cls)]


def twins(C, cls):
    """The aligned row of width C and its base-shifted variants: the same call but for the operands' alignment."""
    rows = [c for c in CASES if c.C == C and c.cls == cls and c.group in ("width", "base")]
    aligned = [c for c in rows if c.x_shift == 0 and c.out_shift == 0]
    assert len(aligned) == 1
    return aligned[0], [c for c in rows if c is not aligned[0]]
