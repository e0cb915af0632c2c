"""Named frames and parameters for the directional rain-streak removal
(csrc/derain.hip), shared by test_streak_cpu.py (which proves each case's
regime on tests/streak_ref.py alone) and test_streak_gpu.py (which pins the
kernels to it).  A helper, not a test.

The kernels' own edges, one pixel either side of each: the 64 x 64 tile of the
line kernels with its halo of n / 2 rows and of the line's reach in columns,
the 1024-pixel segment of the row kernel with its halo of width - 1 columns,
the 4-pixel words of every kernel and the 16-pixel plane pitch."""
import functools

import numpy as np

from streak_ref import offset, streak_ref


def road(H, W, seed):
    """A noisy road-like frame without thin structures: a row gradient
    60 -> 170, a per-channel tint, 30 rectangles of +-40, sigma 6 noise."""
    rng = np.random.default_rng(seed)
    img = np.broadcast_to(np.linspace(60, 170, H)[:, None, None], (H, W, 3)).copy()
    img += rng.normal(0, 12, size=(1, 1, 3))
    for _ in range(30):
        h = int(rng.integers(max(2, H // 40), max(3, H // 6)))
        w = int(rng.integers(max(2, W // 40), max(3, W // 5)))
        y0 = int(rng.integers(0, max(1, H - h)))
        x0 = int(rng.integers(0, max(1, W - w)))
        img[y0:y0 + h, x0:x0 + w] += rng.uniform(-40, 40, size=3)
    img += rng.normal(0, 6, size=img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def smooth(H, W, seed=0):
    """A noise-free tinted gradient: no top-hat response of its own."""
    y, x = np.mgrid[0:H, 0:W]
    img = np.empty((H, W, 3), np.int64)
    img[..., 0] = 50 + (60 * y) // max(H - 1, 1) + 3 * seed
    img[..., 1] = 70 + (50 * x) // max(W - 1, 1)
    img[..., 2] = 90 + (40 * (x + y)) // max(H + W - 2, 1)
    return img.astype(np.uint8)


def noise(H, W, seed, levels=None):
    rng = np.random.default_rng(seed)
    if levels is None:
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    return rng.choice(np.array(levels, np.uint8), size=(H, W, 3))


def sparse(H, W, seed, p):
    """A dark ground of 40 with a share p of single bright pixels (100..255):
    lines form by chance, short ones often and long ones seldom."""
    rng = np.random.default_rng(seed)
    v = np.where(rng.random((H, W)) < p, rng.integers(100, 256, (H, W)), 40)
    img = np.repeat(v[..., None], 3, axis=2)
    img[..., 0] -= 7
    return img.astype(np.uint8)


def flat(H, W, v):
    return np.full((H, W, 3), v, np.uint8)


def line_pixels(H, W, yc, xc, length, slant, width=1):
    """The in-frame pixels of a streak `length` rows long centred on (yc, xc):
    the line of the op's own offsets o_j, `width` pixels wide."""
    ys, xs = [], []
    for j in range(-(length // 2), length - length // 2):
        for d in range(width):
            y, x = yc + j, xc + offset(j, slant) + d
            if 0 <= y < H and 0 <= x < W:
                ys.append(y)
                xs.append(x)
    return np.array(ys, np.int64), np.array(xs, np.int64)


def add_streak(img, yc, xc, length, slant, a256=115, width=1):
    """The generator's model I' = I + (255 - I) a on one streak, a = a256 / 256
    (0.45 is 115 / 256), rounded to nearest."""
    out = img.copy()
    ys, xs = line_pixels(img.shape[0], img.shape[1], yc, xc, length, slant, width)
    if len(ys):
        v = out[ys, xs].astype(np.int64)
        out[ys, xs] = (v + ((255 - v) * a256 + 128) // 256).astype(np.uint8)
    return out


def rainy(base, slant, seed, n=40, lengths=(5, 9, 17, 33, 61, 120), at=()):
    """`base` with n random streaks (lengths, widths 1..3 and strengths drawn)
    and one streak of the second longest length centred on each point of
    `at`."""
    rng = np.random.default_rng(seed)
    H, W = base.shape[:2]
    img = base
    for _ in range(n):
        img = add_streak(img, int(rng.integers(0, H)), int(rng.integers(0, W)),
                         int(rng.choice(lengths)), slant, int(rng.integers(60, 200)),
                         int(rng.integers(1, 4)))
    for (y, x) in at:
        img = add_streak(img, y, x, lengths[-2], slant, 150, 1)
    return img


def saturated(H, W, slant, ground=30):
    """Lines of (251, 255, 255) and of 255 on a dark ground: g = 255, den = 1."""
    img = flat(H, W, ground)
    for i, xc in enumerate(range(4, W, 9)):
        ys, xs = line_pixels(H, W, H // 2, xc, 2 * H, slant)
        img[ys, xs] = (251, 255, 255) if i & 1 else (255, 255, 255)
    return img


P_DEF = dict(slant=-1)
P_BIG = dict(min_len=33, max_len=97)
# points either side of the tile edges (64, 128) and at the frame borders
EDGES_130 = [(63, 63), (64, 64), (65, 65), (63, 65), (0, 0), (0, 129), (129, 0), (129, 129),
             (64, 0), (0, 64), (129, 64), (64, 129), (127, 128), (128, 127)]

# name -> (frame factory, op params as a user writes them)
CASES = {
    # sizes below the windows: w = 15, L = 33, M = 97
    "size_1x1": (lambda: noise(1, 1, 1), dict(width=15, thresh=1, **P_BIG)),
    "size_1x40": (lambda: noise(1, 40, 2), dict(width=15, thresh=1, min_len=3)),
    "size_40x1": (lambda: noise(40, 1, 3), dict(width=3, thresh=1, slant=4, **P_BIG)),
    "size_3x5": (lambda: noise(3, 5, 4), dict(width=15, thresh=1, slant=-4, **P_BIG)),
    "size_16x16": (lambda: noise(16, 16, 5), dict(width=15, thresh=1, slant=2, **P_BIG)),
    "size_3x5_M0": (lambda: noise(3, 5, 4), dict(width=15, thresh=1, slant=-4, min_len=33)),
    "size_16x16_M0": (lambda: noise(16, 16, 5), dict(width=15, thresh=1, slant=2, min_len=33)),
    # streaks over the full height pass an opening longer than the frame
    "size_20x90": (lambda: rainy(smooth(20, 90), 1, 6, 25, (5, 9, 41)), dict(slant=1, min_len=33)),
    "size_20x90_M": (lambda: rainy(smooth(20, 90), 1, 6, 25, (5, 9, 41)), dict(slant=1, **P_BIG)),
    # dense responses: noise with thresh 1 and short lines
    "noise_L3": (lambda: noise(70, 150, 7), dict(thresh=1, min_len=3, slant=-1)),
    "sparse_L3_M5": (lambda: sparse(70, 150, 8, 0.12), dict(thresh=1, min_len=3, max_len=5, slant=3)),
    "sparse_L5_M9": (lambda: sparse(70, 150, 9, 0.12),
                     dict(thresh=1, min_len=5, max_len=9, slant=-2, width=5)),
    "noise_w15": (lambda: noise(67, 131, 10), dict(thresh=1, min_len=3, width=15, slant=1)),
    # the regimes of the op
    "rain_free": (lambda: road(96, 160, 0), P_DEF),
    "flat_128": (lambda: flat(20, 24, 128), {}),
    "flat_white": (lambda: flat(20, 24, 255), dict(thresh=1)),
    "rain_default": (lambda: rainy(road(96, 160, 1), -1, 11, 60, (9, 17, 33)), P_DEF),
    "thr_1": (lambda: rainy(road(70, 150, 2), 0, 12), dict(thresh=1)),
    "thr_255": (lambda: saturated(70, 150, 0, 0), dict(thresh=255)),
    "thr_255_miss": (lambda: saturated(70, 150, 0, 1), dict(thresh=255)),
    "den_1": (lambda: saturated(70, 150, -1), dict(slant=-1, min_len=9)),
    "w3_wide_streaks": (lambda: rainy(smooth(70, 150), -1, 13), dict(width=3, slant=-1)),
    "w15_wide_streaks": (lambda: rainy(smooth(70, 150), -1, 13), dict(width=15, slant=-1)),
    "reject_long": (lambda: rainy(smooth(130, 130), -1, 14, 50, (9, 17, 33, 129)),
                    dict(slant=-1, min_len=9, max_len=49)),
    # every slant at the largest reach: L = 33, M = 97 (48 columns at +-4)
    "slant_-4": (lambda: rainy(smooth(130, 130, 1), -4, 15, at=EDGES_130), dict(slant=-4, **P_BIG)),
    "slant_-1": (lambda: rainy(smooth(130, 130, 2), -1, 16, at=EDGES_130), dict(slant=-1, **P_BIG)),
    "slant_0": (lambda: rainy(smooth(130, 130, 3), 0, 17, at=EDGES_130), dict(slant=0, **P_BIG)),
    "slant_1": (lambda: rainy(smooth(130, 130, 4), 1, 18, at=EDGES_130), dict(slant=1, **P_BIG)),
    "slant_4": (lambda: rainy(smooth(130, 130, 5), 4, 19, at=EDGES_130), dict(slant=4, **P_BIG)),
    "slant_3_noise": (lambda: rainy(road(130, 130, 3), 3, 20, 80), dict(slant=3, thresh=8,
                                                                       min_len=33, max_len=97)),
    "slant_-3": (lambda: rainy(smooth(100, 140, 6), -3, 21, 60), dict(slant=-3, min_len=17,
                                                                     max_len=35)),
    "slant_2": (lambda: rainy(smooth(100, 140, 7), 2, 22, 60), dict(slant=2, min_len=17)),
    # tile edges of the line kernels (64 x 64)
    "tile_63x63": (lambda: rainy(smooth(63, 63), -1, 23, 30), dict(slant=-1, **P_BIG)),
    "tile_64x64": (lambda: rainy(smooth(64, 64), -1, 24, 30), dict(slant=-1, **P_BIG)),
    "tile_65x65": (lambda: rainy(smooth(65, 65), -1, 25, 30), dict(slant=-1, **P_BIG)),
    "tile_129x127": (lambda: rainy(smooth(129, 127), 4, 26, 60), dict(slant=4, **P_BIG)),
    # word and segment edges of the row kernel (1024 outputs, halo w - 1), the plane pitch
    "seg_3x1023": (lambda: noise(3, 1023, 34), dict(thresh=1, min_len=3, width=15)),
    "seg_3x1024": (lambda: noise(3, 1024, 35), dict(thresh=1, min_len=3, width=15)),
    "seg_3x1025": (lambda: noise(3, 1025, 36), dict(thresh=1, min_len=3, width=15)),
    "seg_12x1040": (lambda: rainy(road(12, 1040, 6), 0, 37, 60, (5, 9, 41),
                                  [(6, 1022), (6, 1024), (6, 1026)]), dict(slant=0, thresh=12)),
    "seg_9x255": (lambda: noise(9, 255, 27), dict(thresh=1, min_len=3, width=15)),
    "seg_9x256": (lambda: noise(9, 256, 28), dict(thresh=1, min_len=3, width=15)),
    "seg_9x257": (lambda: noise(9, 257, 29), dict(thresh=1, min_len=3, width=15)),
    "seg_5x530": (lambda: noise(5, 530, 30), dict(thresh=1, min_len=5, width=9, slant=-4)),
    "seg_40x270": (lambda: rainy(road(40, 270, 4), -1, 31, 60, (5, 9, 17, 33), [(20, 255), (20, 256)]),
                   dict(slant=-1, thresh=12)),
    # 3 W no multiple of 16, W no multiple of 4: the loader's partial words
    "tail_40x254": (lambda: rainy(road(40, 254, 5), 1, 32, 60, (5, 9, 17, 33)), dict(slant=1)),
    "tail_66x67": (lambda: sparse(66, 67, 33, 0.1), dict(thresh=1, min_len=3, max_len=5, slant=-4)),
}

# three 96 x 160 frames with the default parameters and slant -1
BATCH = ["rain_free", "rain_default", "batch_saturated"]
CASES["batch_saturated"] = (lambda: saturated(96, 160, -1), P_DEF)


@functools.lru_cache(maxsize=None)
def frame(name):
    img = np.ascontiguousarray(CASES[name][0]())
    assert img.dtype == np.uint8
    img.setflags(write=False)
    return img


def params(name):
    from rvs_amd.preprocess.ops import streak_params
    return streak_params(CASES[name][1])


@functools.lru_cache(maxsize=None)
def reference(name):
    """(out, S, detail) of tests/streak_ref.py, computed once per case."""
    res = streak_ref(frame(name), *params(name), detail=True)
    for a in res[:2]:
        a.setflags(write=False)
    return res
