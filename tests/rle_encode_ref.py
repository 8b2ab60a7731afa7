"""The device encoder's plan (csrc/rle_encode_kernels.hip, segvlad_rle_encode) restated in NumPy, and the masks built to test it.
A plain module (no fixtures): tests/test_rle_encode_host.py holds the model against RleMasks.from_dense on the CPU,
tests/test_gpu_rle_encode.py runs the kernels on the same masks.  Every comparison made with it is exact.

The plan: a UNIT is one (mask, column, block of `rows` rows), numbered column-major u = col * nrb + block.  A CHANGE is a pixel
that differs from the pixel before it in column-major order (pixel 0: from a clear pixel).
  pass 1   per unit (changes, position of the last change or NONE, set pixels); the bit before a unit's first row is the byte above
           it, for row 0 of column c > 0 the last row of column c - 1, for pixel 0 clear
  scan     per mask over its units in order: exclusive sum of the changes = the unit's rank base; running maximum of
           (last change + 1) = the position before the unit's first change; runs = changes + 1, final run = P - last change,
           area = sum of the set pixels; an exclusive sum over the masks = run_offsets
  pass 2   counts[run_offsets[s] + base + j] = p - previous change for the unit's j-th change at p, and the final run last;
           nothing at all when run_offsets[S] > capacity
The kernel packs 32 rows into a word and finds the changes as w ^ ((w << 1) | prev); per row that is bit ^ the bit before."""
import numpy as np

NONE = 0xFFFFFFFF


def encode_model(masks, rows, capacity=None):
    """masks [S, Hm, Wm] (non-zero = set) -> (counts uint32 or None when they do not fit `capacity`, run_offsets int64 [S + 1],
    areas int64 [S])"""
    m = np.asarray(masks) != 0
    S, Hm, Wm = m.shape
    assert rows > 0 and rows % 32 == 0
    P = Hm * Wm
    nrb = -(-Hm // rows)
    U = Wm * nrb
    # ---- pass 1 -----------------------------------------------------------------------------------------------------------
    b = np.zeros((S, Wm, nrb * rows), bool)
    b[:, :, :Hm] = m.transpose(0, 2, 1)                        # [mask][column][row]
    valid = (np.arange(nrb * rows) < Hm).reshape(nrb, rows)
    b = b.reshape(S, Wm, nrb, rows)
    before = np.zeros((S, Wm, nrb), bool)                      # the bit before every unit's first row
    before[:, :, 1:] = b[:, :, :-1, rows - 1]
    before[:, 1:, 0] = m[:, Hm - 1, :-1]                       # row 0 of column c > 0: the end of column c - 1; pixel 0: clear
    prev = np.concatenate([before[..., None], b[..., :-1]], axis=-1)
    t = (b ^ prev) & valid
    unit_n = t.sum(-1).astype(np.uint32)
    row_of_last = (rows - 1) - np.argmax(t[..., ::-1], axis=-1)
    first_pixel = (np.arange(Wm, dtype=np.int64)[:, None] * Hm + np.arange(nrb, dtype=np.int64)[None, :] * rows)[None]
    unit_last = np.where(unit_n > 0, first_pixel + row_of_last, NONE).astype(np.uint32)
    unit_area = (b & valid).sum(-1).astype(np.uint32)
    # ---- scan: the units of a mask in column-major order ------------------------------------------------------------------------
    n = unit_n.reshape(S, U).astype(np.int64)
    key = (unit_last.reshape(S, U) + np.uint32(1)).astype(np.int64)       # NONE + 1 wraps to 0
    base = np.cumsum(n, axis=1) - n
    run = np.maximum.accumulate(key, axis=1) if U else key
    excl = np.concatenate([np.zeros((S, 1), np.int64), run[:, :-1]], axis=1)
    unit_prev = np.where(excl > 0, excl - 1, 0)
    last_key = run[:, -1] if U else np.zeros(S, np.int64)
    n_runs = n.sum(1) + 1
    final_run = P - np.where(last_key > 0, last_key - 1, 0)
    areas = unit_area.reshape(S, U).astype(np.int64).sum(1)
    run_offsets = np.concatenate([[0], np.cumsum(n_runs)]).astype(np.int64)
    total = int(run_offsets[-1])
    if capacity is not None and total > capacity:
        return None, run_offsets, areas
    # ---- pass 2 -----------------------------------------------------------------------------------------------------------------
    counts = np.full(total, NONE, np.uint32)
    si, ui, ri = np.nonzero(t.reshape(S, U, rows))             # every change, by mask, unit, row
    p = first_pixel.reshape(U)[ui] + ri
    flat = si * U + ui
    first_of_unit = np.ones(len(p), bool)
    first_of_unit[1:] = flat[1:] != flat[:-1]
    start = np.maximum.accumulate(np.where(first_of_unit, np.arange(len(p)), 0)) if len(p) else np.zeros(0, np.int64)
    j = np.arange(len(p)) - start
    previous = np.where(first_of_unit, unit_prev[si, ui], np.concatenate([[0], p[:-1]]))
    counts[run_offsets[si] + base[si, ui] + j] = p - previous
    if S:
        counts[run_offsets[1:] - 1] = final_run
    return counts, run_offsets, areas


# ---- masks -------------------------------------------------------------------------------------------------------------------------
RUN_GEOMETRIES = [(64, 96)] + [(Hm, 40) for Hm in (31, 32, 33, 64, 65)]
LANE_WIDTHS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257)      # with Hm = 33: around one lane, one wave of byte lanes, one of 4-byte lanes


def run_structure_masks(Hm, Wm):
    """(uint8 [S, Hm, Wm], names): masks built column-major for the run bookkeeping"""
    P = Hm * Wm
    rng = np.random.Generator(np.random.PCG64(8800 + Hm))
    p = np.arange(P)
    col, row = p // Hm, p % Hm
    flat, names = [], []

    def add(name, f):
        names.append(name)
        flat.append(np.asarray(f, bool))

    add("alternate", p & 1)                                      # P runs
    add("alternate_from_one", (p & 1) == 0)                      # P + 1 runs, the first of length 0: the maximum
    add("checkerboard", (col + row) & 1)
    add("one_whole_column", col == 7)
    add("three_whole_columns", (col >= 2) & (col < 5))
    add("ends_on_column_ends", (row >= 5) & (col % 3 == 0))
    add("starts_on_column_starts", (row < Hm - 4) & (col % 2 == 1))
    add("first_pixel", p == 0)
    add("last_pixel", p == P - 1)
    add("all_but_the_ends", (p > 0) & (p < P - 1))
    f = np.zeros(P, bool)
    f[2 * rng.permutation(P // 2)[:min(300, P // 4)] + 1] = True  # isolated pixels: odd positions, never neighbours
    add("isolated", f)
    dense = np.stack(flat).reshape(len(flat), Wm, Hm).transpose(0, 2, 1)
    vals = rng.choice(np.array([1, 2, 128, 255], np.uint8), size=dense.shape)
    return np.ascontiguousarray(dense * vals), names


def lane_edge_masks(Wm, Hm=33):
    """uint8 [4, Hm, Wm]: random masks at three densities and the alternating mask"""
    rng = np.random.Generator(np.random.PCG64(9900 + Wm))
    m = np.stack([rng.random((Hm, Wm)) < d for d in (0.5, 0.1, 0.9)] + [((np.arange(Hm * Wm) & 1) == 0).reshape(Wm, Hm).T])
    return np.ascontiguousarray(m.astype(np.uint8) * rng.choice(np.array([1, 2, 128, 255], np.uint8), size=m.shape))


def block_edge_masks(rows, Wm):
    """uint8 [S, 2 * rows + 33, Wm]: changes on the rows at each boundary between two row blocks and one row on either side, a set
    last row of a column followed by a set / a clear first row of the next, and random masks"""
    Hm = 2 * rows + 33
    rng = np.random.Generator(np.random.PCG64(6600 + Wm))
    out = []
    for k in (1, 2):
        e = k * rows                                            # the first row of block k
        for lo, hi in ((e - 1, e), (e, e + 1), (e - 2, e - 1), (e - 1, e + 1), (e - 2, e + 2), (e + 1, e + 2), (0, e), (e, Hm)):
            m = np.zeros((Hm, Wm), bool)
            m[lo:hi, :] = True                                  # rows lo .. hi - 1 of every column
            out.append(m)
        m = np.ones((Hm, Wm), bool)
        m[e, :] = False
        out.append(m)
    m = np.zeros((Hm, Wm), bool)                                # column ends: (set last row, set first row), (set last row, clear first row)
    m[Hm - 1, :] = True
    m[0, 1::2] = True
    out.append(m)
    m = np.zeros((Hm, Wm), bool)
    m[Hm - 1, 0] = True
    out.append(m)
    m = np.ones((Hm, Wm), bool)
    m[Hm - 1, :] = False
    out.append(m)
    out += [rng.random((Hm, Wm)) < d for d in (0.5, 0.05)]
    m = np.stack(out)
    return np.ascontiguousarray(m.astype(np.uint8) * rng.choice(np.array([1, 2, 128, 255], np.uint8), size=m.shape))
