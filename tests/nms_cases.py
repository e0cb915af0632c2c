"""The named inputs of the NMS path tests (test_nms_cases_cpu.py,
test_nms_paths_gpu.py): every case is one launch of rv_nms_postprocess (after
rv_candidates_from_raw where the input is a raw prediction) with the oracle's
answer (oracle/yolo_ref.postprocess, computed once) and, from the oracle side
alone, the regime the greedy pass ran in (greedy_regime: an instrumented
numpy restatement of torchvision's CPU nms that must agree with cpu.nms on
every case).  test_nms_cases_cpu.py asserts the regimes, so the GPU tests
cannot silently run another path of csrc/nms.hip than the one a case is named
for: rank sort up to 1024 candidates and bitonic beyond, keys in LDS up to
4096 and in the workspace beyond, chunks of 64 sorted candidates, 16 waves
striding over the kept list.

An image is either a raw prediction (4 + nc, A) or a hand-built segmented
candidate layout: `Cand` rows of 32 B (x1, y1, x2, y2, score f32; cls, anchor,
pad i32), nseg segments of 64 slots, seg_n rows used per segment; every
unused slot holds POISON.  For a hand-built layout the oracle gets the rows in
slot order as a raw prediction with one anchor per row (the rows' corners are
computed from (cx, cy, w, h) in f32 exactly as postprocess does, so both
sides see the same bits)."""
import functools
from typing import List, NamedTuple, Optional

import numpy as np

from oracle import cpu, yolo_ref

f32 = np.float32
DEFAULTS = dict(conf=0.25, iou=0.7, max_det=300, max_nms=30000, max_wh=7680.0, classes_keep=(),
                img1_hw=(384, 640), img0_hw=(1080, 1920))
# an unused slot: were it read, it would sort first and suppress all of class 0
POISON = (-1e6, -1e6, 1e6, 1e6, np.inf)
SORT_SIZES = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 4095, 4096, 4097]
MIXED_N = [0, 5000, 37, 6000, 1500, 4096]
THRESHOLDS = {"0.5": 0.5, "0.6": 0.6, "0.3": 0.3, "0.7": 0.7}
THR_CLASSES = [0, 5, 79]
# [0, 0, W, 1] and [s, 0, s + W, 1]: inter W - s, union W + s (small integers:
# the f32 quotient is the correctly rounded ratio, i.e. np.float32(thr))
THR_PAIRS = {"0.5": (3, 1), "0.6": (4, 1), "0.3": (13, 7), "0.7": (17, 3)}
THR_SCALE = 100   # the pairs just off the threshold: the same pair x 100, s -+ 1/16 px
SEG_PATTERN = [0, 64, 1, 0, 17, 64, 0, 33, 63, 2]


class Case(NamedTuple):
    name: str
    nc: int
    p: dict                         # DEFAULTS keys
    oracle_raw: List[np.ndarray]    # per image (4 + nc, A_b): what postprocess gets
    raw: Optional[np.ndarray]       # (B, 4 + nc, A) for the device, or None
    cand: Optional[np.ndarray]      # (B, cap, 8) f32 words of hand-built Cand rows, or None
    seg_n: Optional[np.ndarray]     # (B, nseg) i32 as handed to the device (unclamped)
    cap: int
    nseg: int
    note: dict                      # what the generator planted (sorted positions, anchors ...)

    @property
    def B(self):
        return len(self.oracle_raw)


# ---------------------------------------------------------------------------
# box generators (coordinates on a 1/4 px grid: every sum and difference below
# is exact in f32, with or without a class offset)
# ---------------------------------------------------------------------------
def grid_boxes(loc, rng):
    """One box per location index: 16-19 px boxes on a 24 px lattice of 26
    columns, so boxes of different locations never overlap."""
    loc = np.asarray(loc)
    col, row = loc % 26, loc // 26
    j = rng.integers(0, 13, (len(loc), 4)) * 0.25
    x1, y1 = 4 + 24 * col + j[:, 0], 4 + 24 * row + j[:, 1]
    return np.stack([x1, y1, x1 + 16 + j[:, 2], y1 + 16 + j[:, 3]], 1)


def desc_scores(n, lo=0.3, hi=0.95):
    """n distinct f32 scores, descending with the row index."""
    return (lo + (hi - lo) * (n - np.arange(n) - 0.5) / max(n, 1)).astype(f32)


def spread(n, rng, ncu=8):
    """n boxes that never overlap within a class (class = index % ncu), in
    random score order: every one survives."""
    ids = rng.permutation(n)
    return grid_boxes(ids // ncu, rng), desc_scores(n), ids % ncu


def ranked_clusters(n, group, rng, ncu=8):
    """Rows in score order, cut at random into about n / group runs; the rows
    of a run are one location (each moved by at most 1/4 px: IoU > 0.9), so
    exactly the first row of every run survives and the kept boxes reach
    through the whole sorted list -- a sort error anywhere changes which row
    that is."""
    cl = np.sort(rng.integers(0, -(-n // group), n))
    perm = rng.permutation(cl.max() + 1 if n else 0)
    ids = perm[cl] if n else cl
    box = grid_boxes(np.arange(n // ncu + 1), rng)[ids // ncu]  # the location's box ...
    box = box + rng.integers(0, 2, (n, 4)) * 0.25               # ... moved a little
    return box, desc_scores(n), ids % ncu


def tied(n, g, rng, levels=8, ncu=8, dup=0.1):
    """n rows at n // g locations (members within 1/2 px of each other), the
    scores quantised to `levels` values, and a tenth of the rows exact copies
    of another row (box, class and score).  Row order is random: which member
    of a location survives is decided by anchor order among equal scores."""
    nloc = max(n // g, 1)
    ids = rng.integers(0, nloc, n)
    box = grid_boxes(np.arange(nloc // ncu + 1), rng)[ids // ncu] + rng.integers(0, 3, (n, 4)) * 0.25
    score = (0.3 + 0.64 * rng.integers(0, levels, n) / levels).astype(f32)
    cls = ids % ncu
    nd = int(n * dup)
    src, dst = rng.integers(0, n, nd), rng.integers(0, n, nd)
    box[dst], score[dst], cls[dst] = box[src], score[src], cls[src]
    return box, score, cls


# ---------------------------------------------------------------------------
# case builders
# ---------------------------------------------------------------------------
def raw_image(box, score, cls, nc, A, rng, conf=0.25, anchors=None):
    """A raw prediction (4 + nc, A) whose candidates are exactly the given
    rows, at random anchors in random order (or at `anchors`, row by row);
    every other anchor scores below 0.8 conf in every class."""
    n = len(score)
    raw = np.empty((4 + nc, A), f32)
    raw[0], raw[1] = rng.uniform(0, 640, A), rng.uniform(0, 384, A)
    raw[2:4] = rng.uniform(8, 120, (2, A))
    raw[4:] = rng.uniform(0, 0.8 * conf, (nc, A))
    if anchors is None:
        anchors = rng.permutation(A)[:n]
    a = np.asarray(anchors, np.int64)
    box = np.asarray(box, np.float64).reshape(-1, 4)
    raw[0, a], raw[1, a] = (box[:, 0] + box[:, 2]) / 2, (box[:, 1] + box[:, 3]) / 2
    raw[2, a], raw[3, a] = box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]
    raw[4 + np.asarray(cls, np.int64), a] = score
    return raw


def raw_case(name, images, nc, A, seed, cap=None, note=None, **p):
    """images: per image (box (n, 4) xyxy, score, cls) or a ready (4 + nc, A) array."""
    rng = np.random.default_rng(seed)
    q = dict(DEFAULTS, **p)
    raws = [im if isinstance(im, np.ndarray) else raw_image(*im, nc, A, rng, q["conf"])
            for im in images]
    nseg = -(-A // 64)
    return Case(name, nc, q, raws, np.stack(raws), None, None, cap or 64 * nseg, nseg, note or {})


def slots_case(name, counts, nc, seed, cap=None, rows=None, note=None, shuffle=False, **p):
    """Hand-built layout.  counts: per image the nseg segment counts as handed
    to the device; the kernel uses min(max(count, 0), 64) rows of a segment.
    rows(n, rng) -> (box, score, cls) of an image's n rows, which go to the
    used slots in random order.  The anchor field is the slot -- or, with
    `shuffle`, random anchors that rise with the oracle's row order while the
    rows sit in the slots in another order (ties follow the anchor field, not
    the slot)."""
    rng = np.random.default_rng(seed)
    q = dict(DEFAULTS, **p)
    counts = np.asarray(counts, np.int32).reshape(len(counts), -1)
    B, nseg = counts.shape
    cap = cap or 64 * nseg
    cand = np.empty((B, cap, 8), f32)
    cand[:, :, :5] = np.asarray(POISON, f32)
    cand.view(np.int32)[:, :, 5:] = 0
    raws = []
    for b in range(B):
        used = np.clip(counts[b], 0, 64)
        n = int(used.sum())
        box, score, cls = (rows or spread)(n, rng)
        order = rng.permutation(n)  # slot order is not score order
        box, score, cls = np.asarray(box, np.float64)[order], score[order], cls[order]
        xywh = np.stack([(box[:, 0] + box[:, 2]) / 2, (box[:, 1] + box[:, 3]) / 2,
                         box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]]).astype(f32)
        r = np.zeros((4 + nc, n), f32)
        r[:4] = xywh
        r[4 + np.asarray(cls, np.int64), np.arange(n)] = score
        raws.append(r)
        slot = np.concatenate([64 * j + np.arange(u) for j, u in enumerate(used)]).astype(np.int64) \
            if n else np.zeros(0, np.int64)
        anchor = slot
        if shuffle:
            anchor = np.sort(rng.permutation(65536)[:n])
            slot = slot[rng.permutation(n)]
        hw, hh = xywh[2] / f32(2), xywh[3] / f32(2)
        cand[b, slot, :5] = np.stack([xywh[0] - hw, xywh[1] - hh, xywh[0] + hw, xywh[1] + hh,
                                      np.asarray(score, f32)], 1)
        ci = cand.view(np.int32)
        ci[b, slot, 5], ci[b, slot, 6] = np.asarray(cls, np.int32), anchor.astype(np.int32)
    return Case(name, nc, q, raws, None, cand, counts, cap, nseg, note or {})


def _sort_rows(n, rng):
    """Distinct scores; up to 1025 rows all survive, beyond that clusters of
    ceil(n / 1000) rows in score order leave about 1000 survivors that reach
    to the end of the sorted list (so max_det = 1024 cuts nothing off)."""
    return spread(n, rng) if n <= 1025 else ranked_clusters(n, -(-n // 1000), rng)


def _place(n, rng, planted, ncu=8):
    """n rows in score order: the planted {sorted position: (box, cls)} and
    non-overlapping fillers elsewhere (locations 200+: clear of the planted
    boxes, which stay inside 0..4000 x 0..100 px of classes >= 0)."""
    ids = rng.permutation(n)
    box, cls = grid_boxes(200 + ids // ncu, rng), ids % ncu
    for pos, (bx, c) in planted.items():
        box[pos], cls[pos] = bx, c
    return box, desc_scores(n), cls


def _chain(x0, y0=0.0):
    """a suppresses b (IoU 7/13), b would suppress c, a does not (4/16), at iou 0.5."""
    return [np.array([x0 + 3.0 * k, y0, x0 + 3.0 * k + 10.0, y0 + 10.0]) for k in range(3)]


def _kept_growth(rng, chunks=6, new=20, ncu=8):
    """Sorted rows of `chunks` chunks of 64: `new` fresh boxes per chunk and
    64 - new exact copies of kept boxes -- in chunk 0 of its own fresh boxes
    (suppressed inside the chunk), later of the kept boxes of earlier chunks,
    kept index 7 t mod (kept so far): every residue mod 16 is a suppressor."""
    box, cls = np.zeros((64 * chunks, 4)), np.zeros(64 * chunks, np.int64)
    kept = []  # (box, cls) in kept order
    t = 0
    for c in range(chunks):
        ids = c * new + np.arange(new)
        fresh = list(zip(grid_boxes(ids // ncu, rng), ids % ncu))
        before = len(kept)
        pos = np.arange(64) if c == 0 else rng.permutation(64)
        order = np.sort(pos[:new])  # fresh boxes keep their order: kept index = order of position
        for k, q in enumerate(order):
            box[64 * c + q], cls[64 * c + q] = fresh[k]
        for q in pos[new:]:
            src = fresh[t % new] if c == 0 else kept[(7 * t) % before]
            box[64 * c + q], cls[64 * c + q] = src
            t += 1
        kept += fresh
    return box, desc_scores(64 * chunks), cls


def _thr_rows(key, c):
    """Three pairs of class c, 40 px apart in y: IoU just below, exactly at
    and just above the threshold `key`; scores descending, pair by pair."""
    W, s = THR_PAIRS[key]
    k, e = THR_SCALE, 1.0 / 16
    rows = []
    for i, (w, sh) in enumerate([(W * k, s * k + e), (W, s), (W * k, s * k - e)]):
        y = 40.0 * i
        rows += [[0, y, w, y + 1], [sh, y, sh + w, y + 1]]
    return np.array(rows, np.float64), desc_scores(6), np.full(6, c)


def _edge_rows(rng, w1, h1):
    """Boxes inside the letterboxed image and boxes that run past each edge."""
    c, wh = rng.uniform([0, 0], [w1, h1], (40, 2)), rng.uniform(20, 90, (40, 2))
    box, score, cls = np.concatenate([c - wh / 2, c + wh / 2], 1), desc_scores(40), \
        rng.integers(0, 9, 40)
    over = np.array([[-30, 10, 40, 60], [w1 - 20, 10, w1 + 50, 60], [100, -25, 160, 30],
                     [100, h1 - 10, 160, h1 + 40], [-50, -50, w1 + 50, h1 + 50],
                     [-90, 5, -20, 50], [w1 + 5, 5, w1 + 60, 50]], np.float64)
    k = len(over)
    box[:k], cls[:k] = over, 9
    return box, score, cls


def _cand_raw(nc, A, B, rng, conf):
    """Raw predictions for the candidate kernel: about 30 % of the anchors
    pass; planted in every image at anchors 1, 2, 3, 5 (see the note)."""
    raw = np.empty((B, 4 + nc, A), f32)
    raw[:, 0], raw[:, 1] = rng.uniform(0, 640, (B, A)), rng.uniform(0, 384, (B, A))
    raw[:, 2:4] = rng.uniform(8, 120, (B, 2, A))
    raw[:, 4:] = rng.uniform(0, 0.8 * conf, (B, nc, A))
    for b in range(B):
        a = np.nonzero(rng.uniform(0, 1, A) < 0.3)[0]
        raw[b, 4 + rng.integers(0, nc, len(a)), a] = rng.uniform(conf + 0.01, 0.95, len(a))
        c32 = f32(conf)
        raw[b, 4:, 1] = 0
        raw[b, 4 + (b % nc), 1] = c32                            # == conf: rejected
        raw[b, 4:, 2] = 0
        raw[b, 4 + nc - 1, 2] = np.nextafter(c32, f32(1))        # accepted; the best class is the last
        raw[b, 4:, 3] = 0
        raw[b, 4 + nc // 3, 3] = raw[b, 4 + nc - 1, 3] = f32(0.625)  # tie: the lower class id (nc > 1)
        raw[b, 4:, 5] = c32                                      # every class == conf: rejected
    return raw


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case.  Seeds and sizes were chosen on the oracle alone, for the
    regimes that test_nms_cases_cpu.py asserts."""
    out = []
    R = np.random.default_rng

    # --- sort algorithm and key store: n on either side of every boundary
    for n in SORT_SIZES:
        A = max(64, -(-(n + n // 3 + 7) // 64) * 64 + (13 if n in (65, 1025) else 0))
        out.append(raw_case(f"sort_n{n}", [_sort_rows(n, R(100 + n))], 8, A, seed=n, max_det=1024))
    out.append(slots_case("sort_full_65536", [[64] * 1024], 8, seed=7, max_det=1024, max_nms=65536,
                          rows=lambda n, rng: ranked_clusters(n, 66, rng)))

    # --- ties under each sorter
    for n, g in [(300, 1), (3000, 3), (6000, 6)]:
        out.append(raw_case(f"ties_n{n}", [tied(n, g, R(200 + n))], 8, 64 * (-(-n // 50)),
                            seed=n, max_det=1024))
    box, _, cls = spread(1500, R(21))
    out.append(raw_case("ties_all_equal_1500", [(box, np.full(1500, 0.5, f32), cls)], 8, 2048,
                        seed=22, max_det=1024))

    # --- max_nms
    out.append(raw_case("max_nms_1", [spread(200, R(31))], 8, 256, seed=31, max_nms=1))
    out.append(raw_case("max_nms_100_in_tie", [tied(400, 1, R(32))], 8, 512, seed=32, max_nms=100))
    out.append(raw_case("max_nms_n_minus_1", [spread(333, R(33))], 8, 400, seed=33, max_nms=332,
                        max_det=1024))
    out.append(raw_case("max_nms_n", [spread(333, R(33))], 8, 400, seed=33, max_nms=333,
                        max_det=1024))
    out.append(raw_case("max_nms_4500_of_5000", [ranked_clusters(5000, 5, R(35))], 8, 6400,
                        seed=35, max_nms=4500, max_det=1024))

    # --- greedy pass
    planted, lanes = {}, [(0, 1, 2), (30, 31, 32), (61, 62, 63)]
    for k, ln in enumerate(lanes):
        for q, bx in zip(ln, _chain(100.0 * k)):
            planted[q] = (bx, 0)
    out.append(raw_case("chain_in_chunk", [_place(64, R(41), planted)], 8, 100, seed=41, iou=0.5,
                        note={"chains": lanes}))
    planted = {q: (bx, 3) for q, bx in zip((10, 69, 70), _chain(0.0))}
    out.append(raw_case("chain_across_chunks", [_place(128, R(42), planted)], 8, 192, seed=42,
                        iou=0.5, note={"chains": [(10, 69, 70)]}))
    out.append(raw_case("kept_growth", [_kept_growth(R(43))], 8, 640, seed=43, max_det=1024))
    same = np.tile([[50.0, 60.0, 150.0, 140.0]], (8, 1))
    out.append(raw_case("classes_never_meet", [(same, desc_scores(8), np.arange(8))], 8, 64,
                        seed=44))
    rng = R(45)
    ctr = rng.uniform(100, 500, (25, 2)).repeat(8, 0) + rng.uniform(-4, 4, (200, 2))
    wh = rng.uniform(30, 40, (200, 2))
    out.append(raw_case("class_126_127", [(np.concatenate([ctr - wh / 2, ctr + wh / 2], 1),
                                           desc_scores(200), 126 + rng.integers(0, 2, 200))],
                        128, 256, seed=45))
    # per kind four sorted rows at one place: the degenerate box, a normal box
    # N around it, the degenerate box again, a copy of N -- only the copy goes
    planted = {}
    for k, d in enumerate([[10, 0, 10, 30], [0, 10, 40, 10], [10, 10, 10, 10], [30, 0, 24, 30]]):
        sh = np.array([60.0 * k, 0, 60.0 * k, 0])
        nb = np.array([0.0, 0, 40, 30]) + sh
        for q, bx in enumerate([np.array(d, np.float64) + sh, nb, np.array(d, np.float64) + sh, nb]):
            planted[4 * k + q] = (bx, 0)
    out.append(raw_case("degenerate_boxes", [_place(64, R(46), planted)], 8, 128, seed=46))

    # --- max_det
    out.append(raw_case("max_det_1", [spread(200, R(51))], 8, 256, seed=51, max_det=1))
    out.append(raw_case("max_det_7_mid_chunk", [tied(200, 4, R(52), levels=64)], 8, 256, seed=52,
                        max_det=7))
    out.append(raw_case("max_det_64_chunk_end", [spread(200, R(53))], 8, 256, seed=53, max_det=64))
    out.append(raw_case("max_det_100", [spread(300, R(54))], 8, 384, seed=54, max_det=100))
    out.append(raw_case("max_det_1024_lds", [spread(3000, R(55))], 8, 4096, seed=55, max_det=1024))
    out.append(raw_case("max_det_1024_ws", [spread(5000, R(56))], 8, 6400, seed=56, max_det=1024))

    # --- class filter
    rng = R(61)
    box, score, _ = spread(300, rng, ncu=1)
    cls = rng.choice([3, 40, 70, 127, 2, 35, 41, 69, 96, 126], 300)
    out.append(raw_case("class_mask_four_words", [(box, score, cls)], 128, 384, seed=61,
                        classes_keep=(3, 40, 70, 127), max_det=1024))
    box, score, _ = spread(300, rng, ncu=1)
    out.append(raw_case("filter_after_max_det", [(box, score, (rng.uniform(0, 1, 300) < 0.1) * 1)],
                        2, 384, seed=62, classes_keep=(1,), max_det=50))

    # --- IoU exactly at the threshold, and just off it
    for key, thr in THRESHOLDS.items():
        out.append(raw_case(f"iou_at_{key}", [_thr_rows(key, c) for c in THR_CLASSES], 80, 64,
                            seed=70, iou=thr, note={"key": key}))

    # --- scale_boxes
    for name, hw0, hw1 in [("landscape", (1080, 1920), (384, 640)),
                           ("portrait", (1920, 1080), (640, 384)),
                           ("square_640", (640, 640), (640, 640)),
                           ("square_1280", (1280, 1280), (640, 640))]:
        out.append(raw_case(f"scale_{name}", [_edge_rows(R(81), hw1[1], hw1[0])], 10, 100, seed=81,
                            img1_hw=hw1, img0_hw=hw0))

    # --- candidate kernel
    for nc, A, B in [(1, 64, 3), (80, 100, 3), (128, 128, 3), (1, 5040, 1), (80, 5040, 3),
                     (128, 5040, 1)]:
        raw = _cand_raw(nc, A, B, R(900 + nc + A), 0.25)
        out.append(raw_case(f"cand_nc{nc}_A{A}", list(raw), nc, A, seed=90, max_det=1024,
                            cap=64 * (-(-A // 64)) + (64 if A == 100 else 0)))

    # --- segmented layout, hand-built
    pat = lambda nseg, k=0: [SEG_PATTERN[(j + k) % len(SEG_PATTERN)] for j in range(nseg)]  # noqa: E731
    out.append(slots_case("slots_nseg1", [[17], [0], [64]], 8, seed=95))
    out.append(slots_case("slots_nseg65", [pat(65), pat(65, 3)], 8, seed=96, max_det=1024))
    out.append(slots_case("slots_nseg1024", [pat(1024)], 8, seed=97, cap=65536, max_det=1024,
                          rows=lambda n, rng: ranked_clusters(n, 28, rng)))
    out.append(slots_case("slots_anchor_order", [pat(65, 5)], 8, seed=94, max_det=1024, shuffle=True,
                          rows=lambda n, rng: tied(n, 2, rng)))
    out.append(slots_case("slots_count_clamp", [[70, -3, 5, 64, -2000000000, 2000000000, 9]], 8,
                          seed=98, cap=512))

    # --- one launch with every kind of image
    mixed = [_sort_rows(n, R(1000 + n)) for n in MIXED_N]
    out.append(raw_case("mixed_batch", mixed, 8, 6400, seed=99, max_det=1024))
    assert len({c.name for c in out}) == len(out)
    return {c.name: c for c in out}


# ---------------------------------------------------------------------------
# the oracle's answer and the regimes
# ---------------------------------------------------------------------------
def candidates(r, conf):
    """The first half of non_max_suppression as yolo_ref.postprocess states
    it: (box (n, 4) f32 xyxy, score, cls, anchor) in anchor order."""
    r = np.asarray(r, f32)
    scores = r[4:]
    anchor = np.nonzero(scores.max(0) > f32(conf))[0] if r.shape[1] else np.zeros(0, np.int64)
    x = r[:, anchor]
    hw, hh = x[2] / f32(2), x[3] / f32(2)
    box = np.stack([x[0] - hw, x[1] - hh, x[0] + hw, x[1] + hh], 1).astype(f32).reshape(-1, 4)
    j = x[4:].argmax(0) if len(anchor) else np.zeros(0, np.int64)
    return box, x[4:][j, np.arange(len(anchor))].astype(f32), j.astype(np.int64), anchor


def greedy_regime(box, score, cls, p):
    """torchvision's CPU nms restated in numpy on the class-offset boxes, as
    far as the kernel runs it (it stops once max_det boxes are kept), with
    counters.  Positions are indices into the sorted, max_nms-cut list."""
    n0 = len(score)
    order = np.argsort(-score, kind="stable")
    ss = score[order]
    _, tie_counts = np.unique(score, return_counts=True) if n0 else (None, np.zeros(1, int))
    n = min(n0, p["max_nms"])
    order = order[:n]
    b = (box + (cls.astype(f32) * f32(p["max_wh"]))[:, None]).astype(f32)[order]
    s = ss[:n]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    thr, thr32, max_det = float(p["iou"]), f32(p["iou"]), p["max_det"]
    sup = np.zeros(n, bool)
    pos = np.arange(n)
    kept, at_chunk, residues = [], [], set()
    cross = inside = at_thr = 0
    for a in range(n):
        if a % 64 == 0:
            if len(kept) >= max_det:
                break
            at_chunk.append(len(kept))
        if sup[a] or len(kept) >= max_det:
            continue
        k = len(kept)
        kept.append(a)
        if a + 1 == n:
            break
        with np.errstate(all="ignore"):
            w = np.maximum(f32(0), np.minimum(b[a, 2], b[a + 1:, 2]) - np.maximum(b[a, 0], b[a + 1:, 0]))
            h = np.maximum(f32(0), np.minimum(b[a, 3], b[a + 1:, 3]) - np.maximum(b[a, 1], b[a + 1:, 1]))
            inter = w * h
            ovr = inter / (area[a] + area[a + 1:] - inter)
        assert ovr.dtype == f32
        live = ~sup[a + 1:]
        hit = (ovr.astype(np.float64) > thr) & live
        at_thr += int(((ovr == thr32) & live).sum())
        same = pos[a + 1:] // 64 == a // 64
        inside += int((hit & same).sum())
        if (hit & ~same).any():
            cross += int((hit & ~same).sum())
            residues.add(k % 16)
        sup[a + 1:] |= hit
    keep_ref = cpu.nms(b, s, thr, max_det)
    last = kept[-1] if kept else -1
    return {
        "n": n0, "n_cut": n, "kept": np.array(kept, np.int64), "keep_ref": keep_ref.astype(np.int64),
        "order": order,
        "survivors": int(len(cpu.nms(b, s, thr, max(n, 1)))), "survivors_after": len(kept),
        "last_kept": last, "last_kept_lane": last % 64 if kept else -1,
        "mid_chunk": bool(kept) and last % 64 != 63,
        "cross_chunk": cross, "in_chunk": inside, "max_kept_at_chunk_start": max(at_chunk, default=0),
        "suppressor_residues": residues, "at_threshold": at_thr,
        "max_tie": int(tie_counts.max()) if n0 else 0,
        "cut_in_tie": bool(n0 > n and ss[n - 1] == ss[n]),
    }


class Answer(NamedTuple):
    out: List[np.ndarray]     # per image (n, 6) f32: yolo_ref.postprocess
    cand: List[tuple]         # per image candidates()
    regime: List[dict]        # per image greedy_regime()


def postprocess(case, raws=None, **over):
    p = dict(case.p, **over)
    return [yolo_ref.postprocess(r[None], p["img1_hw"], p["img0_hw"], p["conf"], p["iou"],
                                 p["max_det"], p["max_nms"], p["max_wh"], p["classes_keep"])[0]
            for r in (case.oracle_raw if raws is None else raws)]


@functools.lru_cache(maxsize=None)
def oracle(name):
    """The Answer of a case.  Computed once per process."""
    case = cases()[name]
    cands = [candidates(r, case.p["conf"]) for r in case.oracle_raw]
    return Answer(postprocess(case), cands, [greedy_regime(*c[:3], case.p) for c in cands])


# ---------------------------------------------------------------------------
# the device's side (used by the GPU tests only): rv_candidates_from_raw and
# rv_nms_postprocess through rvs_amd._lib on buffers of its own -- no engine,
# no weights, no plan
# ---------------------------------------------------------------------------
class Device(NamedTuple):
    out: np.ndarray         # (B, max_det, 6) f32, NaN where the kernel wrote nothing
    out_n: np.ndarray       # (B,)
    cand_total: np.ndarray  # (B,)
    cand: np.ndarray        # (B, cap, 8) f32 words
    seg_n: np.ndarray       # (B, nseg)


def scale5(p):
    from rvs_amd.detect.yolo_hip import scale_boxes_params
    gain, px, py = scale_boxes_params(p["img1_hw"], p["img0_hw"])
    return np.array([gain, px, py, p["img0_hw"][1], p["img0_hw"][0]], f32)


def device_run(case, cuda, images=None, iou_arg=None):
    """One launch over the given images of the case (default: all).  iou_arg:
    the f32 handed to rv_nms_postprocess (default: the product's conversion of
    the configured double, yolo_hip.iou_threshold_f32)."""
    import torch
    from rvs_amd import _lib
    from rvs_amd._lib import call, ptr
    from rvs_amd.detect.yolo_hip import class_mask, iou_threshold_f32
    p = case.p
    idx = list(range(case.B)) if images is None else list(images)
    B, cap, nseg = len(idx), case.cap, case.nseg
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)  # noqa: E731
    if case.raw is not None:
        host = np.empty((B, cap, 8), f32)
        host[:, :, :5] = np.asarray(POISON, f32)
        host.view(np.int32)[:, :, 5:] = 0
        cand = dev(host)
        seg_n = torch.full((B, nseg), -7, dtype=torch.int32, device=cuda)
        raw = dev(case.raw[idx])
        call("rv_candidates_from_raw", ptr(raw), B, case.nc, raw.shape[2], float(p["conf"]),
             ptr(cand), cap, ptr(seg_n), 0)
    else:
        cand, seg_n = dev(case.cand[idx]), dev(case.seg_n[idx])
    md = p["max_det"]
    out = torch.full((B, md, 6), float("nan"), dtype=torch.float32, device=cuda)
    out_n = torch.full((B,), -1, dtype=torch.int32, device=cuda)
    total = torch.full((B,), -1, dtype=torch.int32, device=cuda)
    ws = torch.empty(max(int(_lib.load().rv_nms_ws_bytes(B)), 8), dtype=torch.uint8, device=cuda)
    m = class_mask(p["classes_keep"])
    keep = None if m is None else dev(m.view(np.int32))
    sc = dev(scale5(p))
    iou = iou_threshold_f32(p["iou"]) if iou_arg is None else iou_arg
    call("rv_nms_postprocess", ptr(cand), ptr(seg_n), B, cap, nseg, iou, md, p["max_nms"],
         float(p["max_wh"]), ptr(sc), ptr(keep), ptr(out), ptr(out_n), ptr(total), ptr(ws),
         ws.numel(), 0)
    torch.cuda.synchronize()
    return Device(*(t.cpu().numpy() for t in (out, out_n, total, cand, seg_n)))


def compare(case, dv, images=None):
    """The device's answer against the oracle's, bit for bit."""
    ans = oracle(case.name)
    idx = list(range(case.B)) if images is None else list(images)
    for k, b in enumerate(idx):
        msg = f"{case.name} image {b}"
        ref = ans.out[b]
        assert int(dv.cand_total[k]) == ans.regime[b]["n"], msg
        assert int(dv.out_n[k]) == len(ref), (msg, int(dv.out_n[k]), len(ref))
        np.testing.assert_array_equal(dv.out[k, :len(ref)], ref, err_msg=msg)
        assert dv.out[k, :len(ref)].tobytes() == ref.tobytes(), msg
        assert np.isnan(dv.out[k, len(ref):]).all(), msg  # nothing written past out_n


def compare_candidates(case, dv, images=None):
    """rv_candidates_from_raw's rows and counts against candidates(): segment
    j holds the passing anchors of [64 j, 64 j + 64) in anchor order; every
    other slot is untouched."""
    ans = oracle(case.name)
    idx = list(range(case.B)) if images is None else list(images)
    for k, b in enumerate(idx):
        msg = f"{case.name} image {b}"
        box, score, cls, anchor = ans.cand[b]
        cnt = np.bincount(anchor // 64, minlength=case.nseg).astype(np.int32)
        np.testing.assert_array_equal(dv.seg_n[k], cnt, err_msg=msg)
        first = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        slot = 64 * (anchor // 64) + np.arange(len(anchor)) - first[anchor // 64]
        want = np.empty((case.cap, 8), f32)
        want[:, :5] = np.asarray(POISON, f32)
        wi = want.view(np.int32)
        wi[:, 5:] = 0
        want[slot, :4], want[slot, 4] = box, score
        wi[slot, 5], wi[slot, 6] = cls, anchor
        assert dv.cand[k].tobytes() == want.tobytes(), msg
