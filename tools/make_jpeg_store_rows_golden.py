"""Writes tests/golden/jpeg_store_rows.json: what coclr_jpeg_store_index leaves in a store's rows -- per chunk the serial
Huffman decoder's state, block count and DC predictors -- so that a change of jpeg_store_index_kernel is held to the
words it stored before and not only to the frames decoded from them.

    python tools/make_jpeg_store_rows_golden.py     # on an MI355X, on the commit whose rows are to be kept

`stores()` builds, for chunk sizes 8 and 64, a store of the 54 fixtures of tests/golden/jpeg_frames.pt added in index
order, one pack each; the file holds each store's chunk_rows and the SHA-256 of the bytes of its first chunk_rows rows.
tests/test_gpu_jpeg_store.py calls `digests()` again and compares.  At chunk size 8 the store has more than 2048 rows,
so frames of several windows of the indexer, and the carry from one window to the next, are inside the digest."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tests")) if p not in sys.path]

import _jpeg_cases as J                     # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "jpeg_store_rows.json")
CHUNKS = (8, 64)


def stores():
    """chunk size -> a store of the 54 fixtures in index order, each its own pack."""
    from coclr_amd import jpeg
    cases = J.cases()
    assert len(cases) == 54
    out = {}
    for chunk_bytes in CHUNKS:
        store = jpeg.Store(1 << 20, 64, chunk_bytes=chunk_bytes)
        assert [store.add(jpeg.pack([J.raw(c)])) for c in cases] == list(range(54))
        out[chunk_bytes] = store
    return out


def digests():
    out = {}
    for chunk_bytes, store in stores().items():
        rows = store._rows[:store.chunk_rows].cpu().contiguous()
        out[str(chunk_bytes)] = {"chunk_rows": store.chunk_rows,
                                 "sha256": hashlib.sha256(rows.numpy().tobytes()).hexdigest()}
    return out


def main():
    with open(OUT, "w") as f:
        json.dump(digests(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %s" % (OUT, open(OUT).read()))


if __name__ == "__main__":
    main()
