"""numpy restatement of csrc/pk_edit.h, written from the definition: the edit distance of two id
sequences, the walk back with its tie rule, and a brute force over every alignment for tiny pairs.  Nothing here knows how
the engine computes it."""
import numpy as np

HIT, SUB, DEL, INS = 0, 1, 2, 3


def table(ref, hyp):
    """D (N + 1, M + 1) int32: D(i, 0) = i, D(0, j) = j, D(i, j) = D(i - 1, j - 1) on equal ids, else 1 + the smallest of the
    three neighbours.  A row at a time: the minimum over the cell to the left is a running minimum of (value - column)."""
    ref, hyp = np.asarray(ref, dtype=np.int64).reshape(-1), np.asarray(hyp, dtype=np.int64).reshape(-1)
    N, M = ref.size, hyp.size
    D = np.zeros((N + 1, M + 1), dtype=np.int32)
    D[0] = np.arange(M + 1)
    cols = np.arange(M + 1, dtype=np.int64)
    for i in range(1, N + 1):
        eq = ref[i - 1] == hyp
        # without the cell to the left: c(j) for j >= 1, c(0) = i
        c = np.empty(M + 1, dtype=np.int64)
        c[0] = i
        c[1:] = np.where(eq, D[i - 1, :-1], 1 + np.minimum(D[i - 1, :-1], D[i - 1, 1:]))
        # D(i, j) = min(c(j), D(i, j - 1) + 1) wherever the ids differ; on equal ids c(j) = D(i - 1, j - 1) <= D(i, j - 1) + 1
        # holds anyway (neighbouring cells differ by at most 1), so the running minimum is the definition for every j
        D[i] = np.minimum.accumulate(c - cols) + cols
    return D


def table_slow(ref, hyp):
    """The same, cell by cell, exactly as the definition reads (for the small pairs of the CPU tests)."""
    N, M = len(ref), len(hyp)
    D = np.zeros((N + 1, M + 1), dtype=np.int32)
    for i in range(N + 1):
        D[i, 0] = i
    for j in range(M + 1):
        D[0, j] = j
    for i in range(1, N + 1):
        for j in range(1, M + 1):
            if ref[i - 1] == hyp[j - 1]:
                D[i, j] = D[i - 1, j - 1]
            else:
                D[i, j] = 1 + min(D[i - 1, j - 1], D[i - 1, j], D[i, j - 1])
    return D


def distance(ref, hyp):
    return int(table(ref, hyp)[-1, -1])


def walk(ref, hyp, D):
    """The ops in forward order (uint8) from D by the rule of pk_edit.h."""
    i, j = len(ref), len(hyp)
    ops = []
    while i > 0 or j > 0:
        if i == 0:
            op = INS
        elif j == 0:
            op = DEL
        elif ref[i - 1] == hyp[j - 1]:
            op = HIT
        elif D[i - 1, j - 1] == D[i, j] - 1:
            op = SUB
        elif D[i - 1, j] == D[i, j] - 1:
            op = DEL
        else:
            assert D[i, j - 1] == D[i, j] - 1
            op = INS
        ops.append(op)
        i -= op != INS
        j -= op != DEL
    return np.array(ops[::-1], dtype=np.uint8)


def align(ref, hyp, slow=False):
    """-> dict(distance, ops (P,) uint8, length P, counts (4,) int32: hits, substitutions, deletions, insertions)."""
    ref, hyp = [int(v) for v in np.asarray(ref).reshape(-1)], [int(v) for v in np.asarray(hyp).reshape(-1)]
    D = table_slow(ref, hyp) if slow else table(ref, hyp)
    ops = walk(ref, hyp, D)
    return dict(distance=int(D[-1, -1]), ops=ops, length=int(ops.size),
                counts=np.bincount(ops, minlength=4).astype(np.int32))


def index_pairs(ops):
    """ref and hyp index of every step, -1 at a gap."""
    ri, hi, i, j = [], [], 0, 0
    for op in ops:
        ri.append(i if op != INS else -1)
        hi.append(j if op != DEL else -1)
        i += op != INS
        j += op != DEL
    return np.array(ri, dtype=np.int64), np.array(hi, dtype=np.int64)


def all_alignments(ref, hyp):
    """Every monotone alignment of a tiny pair as a tuple of ops in forward order: a diagonal step is a hit on equal ids and a
    substitution otherwise."""
    N, M = len(ref), len(hyp)
    out = []

    def go(i, j, ops):
        if i == N and j == M:
            out.append(tuple(ops))
            return
        if i < N and j < M:
            go(i + 1, j + 1, ops + [HIT if ref[i] == hyp[j] else SUB])
        if i < N:
            go(i + 1, j, ops + [DEL])
        if j < M:
            go(i, j + 1, ops + [INS])
    go(0, 0, [])
    return out


def cost(ops):
    return sum(1 for op in ops if op != HIT)


def plant(rng, ref, n_edits, alphabet):
    """A copy of ``ref`` with ``n_edits`` edits (substitution, deletion, insertion in turn at random places) -> (hyp, n_edits)."""
    hyp = [int(v) for v in ref]
    for e in range(n_edits):
        kind = e % 3
        if kind == 0 and hyp:
            hyp[int(rng.integers(len(hyp)))] = int(rng.integers(alphabet))
        elif kind == 1 and hyp:
            del hyp[int(rng.integers(len(hyp)))]
        else:
            hyp.insert(int(rng.integers(len(hyp) + 1)), int(rng.integers(alphabet)))
    return np.array(hyp, dtype=np.int32), n_edits
