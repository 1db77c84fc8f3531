#!/usr/bin/env python3
"""Generate tests/golden/ingest.npz with PIL: what upstream's `Resize(size)` + `CenterCrop(size)` give for the cases of
tests/_ingest_ref.py (CASES).

    python tests/golden/make_ingest_golden.py

Needs Pillow only.  For every case the file holds `<name>/out`: `Image.resize((ow, oh), BILINEAR)` cropped, as [C][size][size]
uint8, the PIL version that made it, and the source: `<name>/src` ([h][w][C] uint8) for the seeded sources of up to 8 KiB, the
CRC-32 of the bytes (`<name>/crc`) for every source -- the larger ones are rebuilt from their seed by `case_source` and checked
against it, which keeps the file at a few tens of KB.  The fixture pins the result against another PIL on another machine.
"""
from __future__ import annotations

import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from _ingest_ref import CASES, case_source, pil_resize_crop, resize_crop  # noqa: E402

STORE_SRC_UP_TO = 8 << 10


def main():
    import PIL
    out = {"pil_version": np.array(PIL.__version__)}
    for name, (h, w, C, size, fill) in CASES.items():
        src = case_source(name)
        want = pil_resize_crop(src, size)
        assert want.shape == (C, size, size) and want.dtype == np.uint8
        assert np.array_equal(resize_crop(src, size), want), f"{name}: the restatement differs from PIL {PIL.__version__}"
        out[name + "/out"] = want
        out[name + "/crc"] = np.array(zlib.crc32(src.tobytes()), dtype=np.uint32)
        if fill is None and src.size <= STORE_SRC_UP_TO:
            out[name + "/src"] = src
    path = os.path.join(HERE, "ingest.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(CASES)} cases, PIL {PIL.__version__}")


if __name__ == "__main__":
    main()
