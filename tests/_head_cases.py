"""Case tables of the exact contrastive-head tests (tests/test_gpu_head_exact.py, tests/test_gpu_loss_exact.py), as
plain data.  tests/test_head_cases_cpu.py re-derives the launcher branch of every row from the host predicates of
coclr_amd/csrc/nce.hip, loss.hip and retrieval.hip and asserts that every branch is reached; the shapes are the smallest
that reach it."""
from collections import namedtuple

# ---- coclr_gemm ----------------------------------------------------------------------------------------------------------
# C[M][N] (+)= act(alpha * A[M][K] B[K][N] + bias); ta / tb: the operand is stored transposed (m- / k-contiguous);
# pad: extra floats per operand row and per row of C; splits as requested (the launcher may shrink it)
Gemm = namedtuple("Gemm", "name M N K ta tb splits alpha bias relu accumulate pad")

LAYOUTS = ((False, False), (True, False), (False, True), (True, True))
ALPHAS = (1.0, 0.5, 0.125)


def _gemm_rows():
    rows, i = [], 0

    def add(tag, M, N, K, ta, tb, splits=1, accumulate=False, relu=None, pad=None, alpha=None, bias=True):
        nonlocal i
        pad = (0, 5, 3)[i % 3] if pad is None else pad
        if pad == 0 and ((ta and M == 1) or (tb and K == 1)):
            pad = 5                          # a transposed operand of one row is only told apart by its padding
        rows.append(Gemm("%s-%dx%dx%d-%s%s-s%d" % (tag, M, N, K, "t" if ta else "n", "t" if tb else "n", splits),
                         M, N, K, ta, tb, splits, ALPHAS[i % 3] if alpha is None else alpha, bias,
                         bool(i % 2) if relu is None else relu, accumulate, pad))
        i += 1

    for ta, tb in LAYOUTS:
        for M in (1, 31, 32, 33, 65):
            add("m", M, 33, 33, ta, tb)
        for N in (1, 127, 128, 129, 300):
            add("n", 5, N, 33, ta, tb)
    for j, K in enumerate((1, 31, 32, 33, 70, 515)):
        ta, tb = LAYOUTS[j % 4]
        add("k", 7, 33, K, ta, tb)
    for ta, tb in LAYOUTS:                   # more than one tile both ways, rows padded
        add("pad", 33, 129, 70, ta, tb, pad=7)
    # split-K: a last partial slice, a request that shrinks (to 2, to 1), the large-K row
    add("split", 33, 130, 515, True, True, splits=4)
    add("split", 5, 100, 70, False, True, splits=2)
    add("split", 33, 129, 515, False, False, splits=4)
    add("split", 7, 33, 70, True, False, splits=2)
    add("shrink", 9, 40, 40, False, True, splits=4)
    add("shrink", 9, 40, 20, False, False, splits=4)
    add("large", 32, 128, 16384, False, True, splits=128, pad=0)
    # accumulate onto an integer c, direct and folded, ReLU on and off
    for splits in (1, 2):
        for relu in (False, True):
            add("acc-relu" if relu else "acc", 33, 129, 70, False, True, splits=splits, accumulate=True, relu=relu,
                alpha=0.5, pad=3)
    add("acc", 5, 40, 33, True, False, splits=1, accumulate=True, relu=False, alpha=1.0, bias=False, pad=0)
    return rows


GEMM = _gemm_rows()

# ---- coclr_gemm_fused ----------------------------------------------------------------------------------------------------
# mode 0 + rowsum: the weight / bias gradient launch (A m-contiguous where ta); 1: ReLU mask from ep_a (lda = N + pad);
# 4: spread over S positions; 2: row normalise; 3: l_pos term + normalise backward (T = 1 / alpha = 1 / f)
Fused = namedtuple("Fused", "name mode M N K ta tb splits S T pad")


def _fused_rows():
    rows = []
    for M in (31, 33, 65):
        for K in (5, 70):
            rows.append(Fused("rowsum-%dx40x%d" % (M, K), 0, M, 40, K, M != 33, False, 1, 0, 0.0, 3 if M == 33 else 0))
    rows.append(Fused("rowsum-33x200x70-ncols2", 0, 33, 200, 70, True, False, 1, 0, 0.0, 0))
    rows.append(Fused("relumask-6x200x70-s4", 1, 6, 200, 70, False, False, 4, 0, 0.0, 3))
    rows.append(Fused("relumask-33x129x20-s1", 1, 33, 129, 20, False, True, 1, 0, 0.0, 5))
    for S in (1, 12):
        rows.append(Fused("expand-6x200x70-s2-S%d" % S, 4, 6, 200, 70, False, False, 2, S, 0.0, 0))
    rows.append(Fused("expand-33x40x20-s1-S12", 4, 33, 40, 20, False, True, 1, 12, 0.0, 0))
    for j, N in enumerate((64, 128, 129, 200, 512)):
        rows.append(Fused("normalize-N%d" % N, 2, 5, N, N, False, True, 3, 0, 0.0, (0, 3)[j % 2]))
        rows.append(Fused("lposbwd-N%d" % N, 3, 6, N, 70, False, True, 2, 0, (0.125, 0.0625)[j % 2], (0, 3)[j % 2]))
    rows.append(Fused("normalize-N128-s1", 2, 33, 128, 128, False, True, 1, 0, 0.0, 0))
    return rows


FUSED = _fused_rows()
FUSED_REJECTED_N = 513           # modes 2 and 3: a row lives in one wave (N <= 512)

# ---- l2norm, logits --------------------------------------------------------------------------------------------------------
L2NORM = [(rows, D) for rows in (1, 3, 4, 5, 33) for D in (1, 63, 64, 65, 128, 200)]

# (B, K, D, T); D = 128 rows run the fused kernel and, through a q view one float off a 16-byte boundary, the fallback
LOGITS = [(B, K, 128, (0.07, 0.5)[(i + j) % 2]) for i, B in enumerate((1, 7, 8, 9, 32, 33, 40))
          for j, K in enumerate((1, 63, 64, 65, 640))]
LOGITS_OTHER_D = [(9, 65, 64, 0.07), (33, 640, 96, 0.5), (9, 65, 256, 0.5), (40, 63, 64, 0.07)]
# (B, K, D, splits), T = 0.125
LOGITS_BWD = [(B, K, 128, s) for B in (6, 33) for K in (65, 640) for s in (1, 5)]

# ---- queue, gather, pull ---------------------------------------------------------------------------------------------------
ENQUEUE_SMALL = (16, 12, 4)                 # D, K, BW: every pointer position 0, 4, 8
ENQUEUE_LARGE = (128, 8256, 4128)           # D * BW > 2048 * 256 threads: the grid-stride loop runs
FILL_I64 = [(12, 4, 8), (12, 5, 7), (1000, 300, 700), (1000, 300, 701)]      # K, BW, ptr (the last: out of range)
ADVANCE = [(12, 4, 0, 4), (12, 4, 8, 0), (12, 5, 10, 3), (8256, 4128, 4128, 0)]   # K, BW, ptr, expected

Copy = namedtuple("Copy", "name row_elems stride_extra shift_in shift_out")
COPY_SIZES = (1, 3, 4, 60, 70001, 262144 + 1200)
GATHER = ([Copy("dense-%d" % n, n, 0, 0, 0) for n in COPY_SIZES] +
          [Copy("strided-%d+%d" % (n, e), n, e, 0, 0) for n, e in ((1, 3), (3, 5), (4, 4), (60, 4), (60, 2), (70001, 3),
                                                           (262144 + 1200, 8))] +
          [Copy("offset-in-%d" % n, n, 0, 1, 0) for n in (4, 60, 262144 + 1200)] +
          [Copy("offset-out-%d" % n, n, 0, 0, 1) for n in (4, 60)] +
          [Copy("offset-both-%d" % n, n, 4, 1, 1) for n in (60, 70001)])
GATHER_INDEX = (5, 0, 3, 3, 1, 5)           # out of order, repeated; 6 source rows
PULL = ([Copy("aligned-%d" % n, n, 0, 0, 0) for n in COPY_SIZES] +
        [Copy("unaligned-%d" % n, n, 0, 1, 0) for n in (4, 60, 262144 + 1200)])

ELEMENTWISE_N = (1, 255, 600000)            # relu_fwd / relu_bwd: 600000 > 2048 * 256 runs the stride loop
COLSUM = [(rows, cols) for rows in (1, 7) for cols in (1, 255, 257)]

# ---- positives -------------------------------------------------------------------------------------------------------------
# positive_mask on a given similarity matrix / mine_positives on features (D = 128); tied groups are constructed by the
# generators of tests/_head_ref.py from `ties`: sets of columns that hold one value (the row maximum)
TIE_GROUPS = {
    "tiles": (63, 64),                      # two 64-column tiles
    "octets": (3, 12),                      # two octets of one tile
    "wave": (255, 256),                     # positive_mask: thread 255 / thread 0's second stride; wave 3 / wave 0
    "ends": (0, -1),                        # the first and the last column
    "many": (0, 3, 12, 63, 64, 65, 255, 256, -1),   # more tied maxima than topk
}
Mask = namedtuple("Mask", "name B K topk ties")
MASK = ([Mask("B%d-K%d-top%d" % (B, K, t), B, K, t, "many")
         for B, K, t in ((1, 5, 5), (5, 63, 1), (5, 64, 5), (33, 65, 5), (5, 300, 16), (32, 300, 5), (40, 1030, 5),
                         (5, 1030, 16), (5, 300, 0), (33, 5, 0), (1, 1030, 1), (5, 65, 16), (5, 5, 1))] +
        [Mask("ties-%s-K%d-top%d" % (g, K, t), 5, K, t, g)
         for g, K, t in (("tiles", 65, 1), ("tiles", 300, 5), ("octets", 64, 1), ("octets", 300, 5), ("wave", 300, 1),
                         ("wave", 1030, 5), ("ends", 63, 1), ("ends", 1030, 5), ("ends", 300, 16))])
MINE_REJECTED = [(5, 128, 300, 17), (5, 128, 5, 6), (5, 64, 300, 5)]        # B, D, K, topk
MASK_LDS_K = 38401                          # K floats above 150 KiB of LDS: topk > 0 is rejected, topk = 0 runs

Retrieval = namedtuple("Retrieval", "name B N ks")
KS_FULL = (1, 5, 10, 20, 50)
RETRIEVAL = [Retrieval("N50", 5, 50, KS_FULL), Retrieval("N257", 5, 257, KS_FULL), Retrieval("N1000", 4, 1000, KS_FULL),
             Retrieval("N38401", 2, 38401, KS_FULL), Retrieval("N50-k1", 5, 50, (1,)),
             Retrieval("N257-k1", 3, 257, (1,)), Retrieval("N38401-k1", 2, 38401, (1,))]

COLSTATS = [(rows, cols) for rows in (1, 63, 64, 65, 300) for cols in (1, 257)]

# ---- loss ------------------------------------------------------------------------------------------------------------------
# mode 0 InfoNCE (target column), 1 CoCLR multi-positive (+ drop_self), 2 UberNCE
Loss = namedtuple("Loss", "name mode drop_self B N1")
LOSS_MODES = ((0, False), (1, False), (1, True), (2, False))
LOSS = ([Loss("m%d%s-B9-N%d" % (m, "d" if d else "", N1), m, d, 9, N1)
         for m, d in LOSS_MODES for N1 in (1, 2, 77, 255, 256, 257, 1025, 2049)] +
        [Loss("m%d%s-B%d-N%d" % (m, "d" if d else "", B, N1), m, d, B, N1)
         for m, d in LOSS_MODES for B, N1 in ((1, 257), (257, 77))])
