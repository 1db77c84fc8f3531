"""A numpy restatement of the image-folder ingest (include/mdm_ingest.h, csrc/ingest.hip), independent of the C function: PIL's
bilinear `precompute_coeffs` + `normalize_coeffs_8bpc` in Python floats (IEEE double, nothing fused), the two 8-bit passes in int64
with the uint8 rounding between them, and torchvision's `Resize(size)` + `CenterCrop(size)` sizes.  tests/test_ingest_cpu.py checks
it against tests/golden/ingest.npz and against the installed PIL; the GPU tests then check the kernel against all three.

CASES is the list the golden file, the CPU tests and the GPU tests share: name -> (h, w, C, size, fill); fill None = seeded bytes.
GEOMETRY_CASES (below it) are the shapes that reach the other launch geometries of the kernel; tests/test_ingest_geometry_gpu.py
runs them.
"""
import functools
import math
import zlib

import numpy as np

BITS = 22

CASES = {
    "hcrop_37x53": (37, 53, 3, 8, None),            # -> (11, 8, 0, 2): horizontal crop, 159-byte rows
    "vcrop_129x77": (129, 77, 3, 16, None),         # -> (16, 26, 5, 0): vertical crop
    "half_18x16": (18, 16, 3, 8, None),             # top = round(0.5) = 0
    "half_22x16": (22, 16, 3, 8, None),             # top = round(1.5) = 2
    "half_26x16": (26, 16, 3, 8, None),             # top = round(2.5) = 2
    "up_28x28_L": (28, 28, 1, 32, None),            # upsampling, one channel
    "up_crop_17x40": (17, 40, 3, 64, None),         # -> (150, 64, 0, 43): upsampling with a crop
    "identity_16": (16, 16, 3, 16, None),           # identity plans
    "taps37_140x131": (140, 131, 3, 8, None),       # 37 taps
    "taps261_1040x1031": (1040, 1031, 3, 8, None),  # 261 taps, more than a wave has lanes
    "skip_520x37_L": (520, 37, 1, 8, None),         # top 52: a long skipped span
    "const255_37x53": (37, 53, 3, 8, 255),
    "const0_37x53": (37, 53, 3, 8, 0),
}
# what torchvision's Resize + CenterCrop make of some of them: (ow, oh, top, left)
EXPECTED_PLANS = {
    "hcrop_37x53": (11, 8, 0, 2), "vcrop_129x77": (16, 26, 5, 0), "half_18x16": (8, 9, 0, 0), "half_22x16": (8, 11, 2, 0),
    "half_26x16": (8, 13, 2, 0), "up_28x28_L": (32, 32, 0, 0), "up_crop_17x40": (150, 64, 0, 43), "identity_16": (16, 16, 0, 0),
    "skip_520x37_L": (8, 112, 52, 0),
}


# The launch geometries of mdm_ingest_resize_crop that no entry of CASES selects (every one of those is TR = min(S, 8) with the
# horizontal table in LDS and at most 192 (channel, column) pairs): same format, same seeded source.  They are NOT in
# tests/golden/ingest.npz -- some outputs are over a megabyte; their references are the restatement and, where the resized image is
# small enough to build (pil_allowed), the installed PIL.  GEOMETRY_EXPECTED is what each is there for, as mdm_ingest_launch_of must
# report it: (TR, horizontal table in LDS, workgroups per image); tests/test_ingest_cpu.py asks the query, nothing restates the rule.
GEOMETRY_CASES = {
    "preset128": (150, 131, 3, 128, None),          # NJ = 384: a second trip of the lane loops, 16 row tiles, top 9
    "preset256": (300, 270, 3, 256, None),          # NJ = 768: three trips
    "grey264": (280, 300, 1, 264, None),            # one channel past 256 lanes, left 9
    "table_global_830": (830, 830, 3, 500, None),   # the table stays in global memory, 5 taps, last tile 500 mod 8 = 4 rows
    "tr7_33x40": (33, 40, 3, 700, None),            # NJ = 2100 shrinks the row tile to 7; upsampling, left 74
    "wide_12x9000": (12, 9000, 3, 256, None),       # 27 000-byte rows shrink it to 3; last tile 256 mod 3 = 1 row; too large for PIL
    "edge_8x10880": (8, 10880, 3, 16, None),        # TR = 1, 65 512 of 65 536 bytes: the widest row that is accepted
    "narrow_40x3_L": (40, 3, 1, 8, None),           # 3-byte rows: no aligned middle, the head is cut to the row
    "narrow_9x5": (9, 5, 3, 8, None),               # 15-byte rows, three channels
    "one_1x1": (1, 1, 3, 4, None),                  # every tap on the only pixel: the output is constant
}
GEOMETRY_EXPECTED = {
    "preset128": (8, True, 16), "preset256": (8, True, 32), "grey264": (8, True, 33), "table_global_830": (8, False, 63),
    "tr7_33x40": (7, False, 100), "wide_12x9000": (3, False, 86), "edge_8x10880": (1, False, 16), "narrow_40x3_L": (8, True, 1),
    "narrow_9x5": (8, True, 1), "one_1x1": (4, True, 1),
}
PIL_LIMIT = 32 << 20                                 # bytes of the resized image PIL builds before the crop


def pil_allowed(h, w, C, size):
    """Whether the live PIL reference is made for this shape: PIL resizes the WHOLE image before the crop (ow oh C bytes)"""
    ow, oh, _, _ = resize_crop_plan(h, w, size)
    return ow * oh * C < PIL_LIMIT


def case_source(name):
    """The source bytes of a case of CASES or GEOMETRY_CASES, [h][w][C] uint8 (C = 1 keeps its axis): the same on every machine."""
    h, w, C, _, fill = CASES[name] if name in CASES else GEOMETRY_CASES[name]
    if fill is not None:
        return np.full((h, w, C), fill, dtype=np.uint8)
    rng = np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)
    return rng.randint(0, 256, size=(h, w, C)).astype(np.uint8)


def resize_crop_plan(h, w, size):
    """torchvision: Resize(size) keeps the aspect with the SHORTER side at `size` (int() truncates the longer), CenterCrop(size)
    rounds half the excess with Python's round (halves to even).  -> (ow, oh, top, left)"""
    if w <= h:
        ow, oh = size, int(size * h / w)
    else:
        oh, ow = size, int(size * w / h)
    return ow, oh, int(round((oh - size) / 2.0)), int(round((ow - size) / 2.0))


def plan(in_size, out_size, first=0, count=None):
    """-> (ks, bounds [count][2] int32, coeffs [count][ks] int32) for the output positions [first, first + count)"""
    count = out_size - first if count is None else count
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = fs
    ks = 2 * int(math.ceil(support)) + 1
    bounds = np.zeros((count, 2), dtype=np.int32)
    coeffs = np.zeros((count, ks), dtype=np.int32)
    for n, xx in enumerate(range(first, first + count)):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        ws = []
        for x in range(xmax):
            a = abs((x + xmin - center + 0.5) / fs)
            ws.append(1.0 - a if a < 1.0 else 0.0)
        total = 0.0
        for v in ws:
            total += v
        if total != 0.0:
            ws = [v / total for v in ws]
        bounds[n] = (xmin, xmax)
        for x, v in enumerate(ws):
            coeffs[n, x] = int(v * (1 << BITS) - 0.5) if v < 0 else int(v * (1 << BITS) + 0.5)
    return ks, bounds, coeffs


def filter_axis0(img, bounds, coeffs):
    """One 8-bit pass along axis 0: out[n] = clip((2^21 + sum_i img[bounds[n][0] + i] coeffs[n][i]) >> 22, 0, 255) as uint8"""
    out = np.empty((len(bounds),) + img.shape[1:], dtype=np.uint8)
    wide = img.astype(np.int64)
    for n, (lo, cnt) in enumerate(bounds):
        acc = np.full(img.shape[1:], 1 << (BITS - 1), dtype=np.int64)
        for i in range(int(cnt)):
            acc += wide[lo + i] * int(coeffs[n, i])
        out[n] = np.clip(acc >> BITS, 0, 255).astype(np.uint8)
    return out


def resize_crop(src, size):
    """[h][w][C] uint8 -> [C][size][size] uint8: the horizontal pass over the kept columns, its uint8 rounding, the vertical pass
    over the kept rows -- both always run."""
    h, w, _ = src.shape
    ow, oh, top, left = resize_crop_plan(h, w, size)
    _, hb, hc = plan(w, ow, left, size)
    _, vb, vc = plan(h, oh, top, size)
    tmp = filter_axis0(np.ascontiguousarray(src.transpose(1, 0, 2)), hb, hc)          # [size x][h][C]
    out = filter_axis0(np.ascontiguousarray(tmp.transpose(1, 0, 2)), vb, vc)          # [size y][size x][C]
    return np.ascontiguousarray(out.transpose(2, 0, 1))


@functools.lru_cache(maxsize=None)
def geometry_reference(name):
    """A case of GEOMETRY_CASES -> (source, the restatement's output, live PIL's output or None where PIL is not asked): made once
    per process, shared by the tests and read-only"""
    h, w, C, size, _ = GEOMETRY_CASES[name]
    src = case_source(name)
    out = resize_crop(src, size)
    pil = pil_resize_crop(src, size) if pil_allowed(h, w, C, size) else None
    for a in (src, out, pil):
        if a is not None:
            a.setflags(write=False)
    return src, out, pil


def pil_resize_crop(src, size):
    """The same through the installed PIL: what upstream's Resize + CenterCrop give for this image"""
    from PIL import Image
    h, w, C = src.shape
    ow, oh, top, left = resize_crop_plan(h, w, size)
    im = Image.fromarray(src[:, :, 0] if C == 1 else src)
    assert im.mode == ("L" if C == 1 else "RGB")
    out = np.asarray(im.resize((ow, oh), Image.BILINEAR))
    out = out[top:top + size, left:left + size]
    return np.ascontiguousarray(out.reshape(size, size, C).transpose(2, 0, 1))
