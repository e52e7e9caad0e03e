"""Baseline JPEG frames decoded on the GPU, bit-identical to PIL (dataset/lmdb_dataset.py:37-38 of the reference:
`Image.open(BytesIO(raw)).convert('RGB')` with libjpeg-turbo).

    worker:  data, meta = jpeg.pack(raws)                 # headers parsed, tables derived; compressed bytes travel
    collate: data, meta = jpeg.cat(packs)
    loop:    frames = jpeg.decode(data, meta)             # (F, H, W, 3) uint8 on the device

`frames` is what stage_train_clips, stage_classifier_clips, stage_crops and VideoEvaluator.add_frames take.
A batch whose videos differ in frame size (kinetics400-256 keeps every video's aspect ratio) goes through
`cat_ragged` and `decode_ragged` instead, to a staging.RaggedFrames that stage_train_clips_ragged and
stage_classifier_clips_ragged take; `pack`, per video, is the same.
A dataset that fits into the device's memory can stay there compressed: `Store.add(pack)` per video, once, then
`Store.decode(ids)` per step by frame index, to the same RaggedFrames, with nothing but the ids travelling (class Store);
`Store.decode(ids, boxes)` decodes one pixel box of every frame alone, what staging.stage_train_clips_cropped takes.
A dataset larger than the device's memory keeps its bytes in pinned host memory, `Store(..., bytes_on="host")`, and a
built store of either kind is written and read back as data with `Store.save` / `Store.load`.
A dataset that fits the GPUs of a node but not one of them is sharded: each rank's device Store becomes one shard of a
`ShardedStore` (`ShardedStore.join`), mapped into its peers through hipIpc, and `decode` takes global ids.

Scope: baseline / extended sequential Huffman (SOF0, SOF1), 8-bit, one interleaved scan, one component or YCbCr with
luma sampled 1x1, 2x1 or 2x2, optional restart intervals -- what ffmpeg, cv2.imwrite and PIL write by default.
Anything else is refused by `parse` on the host with `Unsupported` (a ValueError naming the reason) before a byte is
uploaded, so a caller can fall back to PIL for that video.

The entropy stage is serial inside a restart segment; with markers every segment is a lane of its own.  A frame
WITHOUT restart markers is one GPU lane (64 frames per wave) on the serial path, `chunk_bytes=0`, or one workgroup with
a lane per chunk of `chunk_bytes` raw bytes: every chunk is decoded from a guessed state and decoded again while its
predecessor's exit state differs from the entry it used, which ends in the serial decoder's own states, so the
frames, `status` and `last_status` are the same bit for bit.  `chunk_bytes=None` takes the policy from the
environment, read per call: COCLR_JPEG_SPLIT=0 serial, =n that chunk size (8..65536); unset is DEFAULT_SPLIT."""
import os

import numpy as np
import torch

from . import ops

META_QUANT, META_HUFF, HUFF_WORDS = 16, 208, 96
META_SEG = META_HUFF + 6 * HUFF_WORDS           # csrc/jpeg_core.h: JM_*
MAX_SIDE = 8192
DEFAULT_SPLIT = 64                               # chunk size when COCLR_JPEG_SPLIT is unset
DEFAULT_STORE_CHUNK = 64                         # a Store's chunk size (PROVISIONAL)

_SOF_NAMES = {0xC2: "progressive (SOF2)", 0xC3: "lossless (SOF3)", 0xC5: "differential sequential (SOF5)",
              0xC6: "differential progressive (SOF6)", 0xC7: "differential lossless (SOF7)",
              0xC9: "arithmetic coding (SOF9)", 0xCA: "arithmetic coding, progressive (SOF10)",
              0xCB: "arithmetic coding, lossless (SOF11)", 0xCD: "arithmetic coding, differential (SOF13)",
              0xCE: "arithmetic coding, differential progressive (SOF14)",
              0xCF: "arithmetic coding, differential lossless (SOF15)"}

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13,
                   6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45,
                   38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


class Unsupported(ValueError):
    """A file this decoder does not take; the message names the reason."""


def _u16(b, at):
    return (b[at] << 8) | b[at + 1]


def parse(raw):
    """The headers of one JPEG file, host only -> dict:
      width, height, ncomp, sampling (hs, vs) of the luma (chroma is 1x1),
      quant: per component its (64,) uint8 table in natural order,
      dc, ac: per component its Huffman table as (bits[16], vals),
      quant_tables, dc_tables, ac_tables: the ids the file defined,
      restart_interval (MCUs, 0 = none), scan = (start, end) byte range of the entropy-coded data,
      segments: offset of every restart segment relative to scan[0].
    Raises Unsupported for everything outside the scope in the module docstring."""
    b = bytes(raw)
    n = len(b)
    if n < 4 or b[0] != 0xFF or b[1] != 0xD8:
        raise Unsupported("not a JPEG file (no SOI)")
    qt, dct, act = {}, {}, {}
    ri, frame, adobe, jfif = 0, None, None, False
    at = 2
    while True:
        if at + 4 > n:
            raise Unsupported("a segment runs past the buffer (file cut before SOS)")
        if b[at] != 0xFF:
            raise Unsupported("garbage between segments at byte %d" % at)
        mk = b[at + 1]
        if mk == 0xFF:                                   # fill byte
            at += 1
            continue
        if mk == 0xD9:
            raise Unsupported("EOI before any scan")
        ln = _u16(b, at + 2)
        if ln < 2 or at + 2 + ln > n:
            raise Unsupported("a segment runs past the buffer (marker FF%02X at byte %d)" % (mk, at))
        seg = b[at + 4:at + 2 + ln]
        if mk in (0xC0, 0xC1):
            if frame is not None:
                raise Unsupported("several frames (a second SOF)")
            if len(seg) < 6 or len(seg) < 6 + 3 * seg[5]:
                raise Unsupported("a short SOF segment")
            if seg[0] != 8:
                raise Unsupported("%d-bit samples" % seg[0])
            frame = {"height": _u16(seg, 1), "width": _u16(seg, 3),
                     "comps": [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i])
                               for i in range(seg[5])]}
        elif mk in _SOF_NAMES:
            raise Unsupported(_SOF_NAMES[mk])
        elif mk == 0xCC:
            raise Unsupported("arithmetic coding (DAC)")
        elif mk == 0xDB:
            i = 0
            while i < len(seg):
                pq, tq = seg[i] >> 4, seg[i] & 15
                if pq != 0:
                    raise Unsupported("16-bit quantisation table")
                if tq > 3 or i + 65 > len(seg):
                    raise Unsupported("a bad DQT segment")
                t = np.zeros(64, dtype=np.uint8)
                t[ZIGZAG] = np.frombuffer(seg, dtype=np.uint8, count=64, offset=i + 1)
                qt[tq] = t
                i += 65
        elif mk == 0xC4:
            i = 0
            while i < len(seg):
                if i + 17 > len(seg):
                    raise Unsupported("a bad DHT segment")
                tc, th = seg[i] >> 4, seg[i] & 15
                bits = np.frombuffer(seg, dtype=np.uint8, count=16, offset=i + 1).astype(np.int64)
                cnt = int(bits.sum())
                if tc > 1 or th > 3 or cnt > 256 or i + 17 + cnt > len(seg):
                    raise Unsupported("a bad DHT segment")
                code = 0
                for l in range(16):                       # the code space must not overflow
                    code = (code + int(bits[l])) << 1
                    if code > (2 << (l + 1)):
                        raise Unsupported("a Huffman table with too many codes")
                vals = np.frombuffer(seg, dtype=np.uint8, count=cnt, offset=i + 17).copy()
                (act if tc else dct)[th] = (bits.copy(), vals)
                i += 17 + cnt
        elif mk == 0xDD:
            if len(seg) != 2:
                raise Unsupported("a bad DRI segment")
            ri = _u16(seg, 0)
        elif mk == 0xEE and len(seg) >= 12 and seg[:5] == b"Adobe":
            adobe = seg[11]
        elif mk == 0xE0 and seg[:5] == b"JFIF\0":
            jfif = True
        elif mk == 0xDC:
            raise Unsupported("DNL (the height is defined after the scan)")
        elif mk == 0xDA:
            break
        at += 2 + ln
    if frame is None:
        raise Unsupported("SOS before any SOF")
    comps, W, H = frame["comps"], frame["width"], frame["height"]
    if len(comps) not in (1, 3):
        raise Unsupported("%d components" % len(comps))
    if H == 0:
        raise Unsupported("DNL (the height is defined after the scan)")
    if W < 1 or W > MAX_SIDE or H > MAX_SIDE:
        raise Unsupported("a %d x %d image (the limit is %d)" % (W, H, MAX_SIDE))
    if len(comps) == 3:
        if adobe == 0:
            raise Unsupported("Adobe APP14 with transform 0 (RGB stored as is)")
        if adobe is None and not jfif and [c[0] for c in comps] == [82, 71, 66]:
            raise Unsupported("components named R, G, B (RGB stored as is)")
        hs, vs = comps[0][1], comps[0][2]
        if (hs, vs) not in ((1, 1), (2, 1), (2, 2)) or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
            raise Unsupported("sampling factors %s" % ", ".join("%dx%d" % (c[1], c[2]) for c in comps))
    else:
        hs, vs = 1, 1                                    # one component is never interleaved: its factors are moot
    # the scan header
    if len(seg) < 1 or len(seg) != 4 + 2 * seg[0]:
        raise Unsupported("a bad SOS segment")
    if seg[0] != len(comps):
        raise Unsupported("several scans (the first holds %d of %d components)" % (seg[0], len(comps)))
    quant, dc, ac = [], [], []
    for i, c in enumerate(comps):
        if seg[1 + 2 * i] != c[0]:
            raise Unsupported("scan components out of frame order")
        td, ta = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
        if c[3] not in qt:
            raise Unsupported("missing quantisation table %d" % c[3])
        if td not in dct:
            raise Unsupported("missing DC Huffman table %d" % td)
        if ta not in act:
            raise Unsupported("missing AC Huffman table %d" % ta)
        quant.append(qt[c[3]])
        dc.append(dct[td])
        ac.append(act[ta])
    ss, se, ah_al = seg[-3], seg[-2], seg[-1]
    if (ss, se, ah_al) != (0, 63, 0):
        raise Unsupported("a scan of part of the spectrum (progressive parameters)")
    start = at + 2 + ln
    # the marker that ends the scan: FF followed by anything but 00, a restart marker or a fill FF
    arr = np.frombuffer(b, dtype=np.uint8, offset=start)
    ff = np.flatnonzero(arr[:-1] == 0xFF) if len(arr) > 1 else np.zeros(0, dtype=np.int64)
    nxt = arr[ff + 1]
    stop = ff[(nxt != 0) & ((nxt < 0xD0) | (nxt > 0xD7)) & (nxt != 0xFF)]
    if len(stop) == 0:
        raise Unsupported("no EOI")
    end = start + int(stop[0])
    last = b[end + 1]
    if last == 0xDC:
        raise Unsupported("DNL (the height is defined after the scan)")
    if last != 0xD9:
        raise Unsupported("several scans (marker FF%02X after the first)" % last)
    rst = ff[(nxt >= 0xD0) & (nxt <= 0xD7) & (ff < end - start)]
    segments = np.concatenate([[0], rst + 2]).astype(np.int64)
    mcus = -(-W // (8 * hs)) * -(-H // (8 * vs))
    want = 1 if ri == 0 else -(-mcus // ri)
    if len(segments) != want:
        raise Unsupported("%d restart segments where the interval of %d MCUs asks for %d" % (len(segments), ri, want))
    return {"width": W, "height": H, "ncomp": len(comps), "sampling": (hs, vs), "quant": quant, "dc": dc, "ac": ac,
            "quant_tables": sorted(qt), "dc_tables": sorted(dct), "ac_tables": sorted(act), "restart_interval": ri,
            "scan": (start, end), "segments": segments}


def _huff_words(table):
    """(bits, vals) -> the 96 words the kernel reads: limit[16], valoff[16], 256 values packed four to a word."""
    bits, vals = table
    w = np.zeros(HUFF_WORDS, dtype=np.int64)
    code, k = 0, 0
    for l in range(16):
        w[16 + l] = k - code                             # value index of a code = valoff + the code itself
        code += int(bits[l])
        k += int(bits[l])
        w[l] = min(code << (15 - l), 65536)
        code <<= 1
    hv = np.zeros(256, dtype=np.uint8)
    hv[:len(vals)] = vals
    w[32:] = hv.view("<u4")
    return w


def _meta_row(info, offset, width):
    m = np.zeros(width, dtype=np.int64)
    m[0], m[1] = offset, info["scan"][1] - info["scan"][0]
    m[2], m[3] = info["restart_interval"], len(info["segments"])
    for c in range(info["ncomp"]):
        m[META_QUANT + 64 * c:META_QUANT + 64 * (c + 1)] = info["quant"][c]
        m[META_HUFF + HUFF_WORDS * c:META_HUFF + HUFF_WORDS * (c + 1)] = _huff_words(info["dc"][c])
        m[META_HUFF + HUFF_WORDS * (3 + c):META_HUFF + HUFF_WORDS * (4 + c)] = _huff_words(info["ac"][c])
    m[META_SEG:META_SEG + len(info["segments"])] = info["segments"]
    # the packed value words are unsigned; store their bit patterns
    return (m & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def pack(raws):
    """JPEG files (bytes-like) of ONE size and sampling -> (data, meta): data uint8 (n,) every frame's entropy-coded
    bytes, meta int32 (F, 8 + width): per frame the kernel's descriptor (include/coclr_hip.h: coclr_jpeg_decode)
    behind 8 words that carry the pack's geometry {8 + width, H, W, components, hs, vs, 0, 0} through a collate.
    Runs in the Dataset worker in place of the PIL decode; raises Unsupported as parse does."""
    raws = list(raws)
    if not raws:
        raise ValueError("coclr_amd: pack needs at least one frame")
    infos = [parse(r) for r in raws]
    key = lambda i: (i["height"], i["width"], i["ncomp"], i["sampling"])     # noqa: E731
    if any(key(i) != key(infos[0]) for i in infos):
        raise Unsupported("frames of one pack differ in size, components or sampling: %s" %
                          sorted(set(key(i) for i in infos)))
    H, W, ncomp, (hs, vs) = key(infos[0])
    width = META_SEG + max(len(i["segments"]) for i in infos)
    meta = np.zeros((len(raws), 8 + width), dtype=np.int32)
    meta[:, :8] = [8 + width, H, W, ncomp, hs, vs, 0, 0]
    chunks, offset = [], 0
    for f, (raw, info) in enumerate(zip(raws, infos)):
        meta[f, 8:] = _meta_row(info, offset, width)
        chunks.append(np.frombuffer(bytes(raw), dtype=np.uint8)[info["scan"][0]:info["scan"][1]])
        offset += len(chunks[-1])
    if offset > 0x7fffffff:
        raise ValueError("coclr_amd: a pack holds up to 2 GiB of compressed bytes")
    data = np.concatenate(chunks) if offset else np.zeros(0, dtype=np.uint8)
    return torch.from_numpy(data.copy()), torch.from_numpy(meta)


def _host_meta(meta):
    if not isinstance(meta, torch.Tensor) or meta.dtype != torch.int32 or meta.dim() != 2 or meta.is_cuda or \
            meta.shape[0] < 1 or meta.shape[1] <= 8 + META_SEG:
        raise ValueError("coclr_amd: meta must be the host int32 (F, width) tensor of jpeg.pack / jpeg.cat_ragged")


def _flat_data(data):
    if not isinstance(data, torch.Tensor) or data.dtype != torch.uint8 or data.dim() != 1:
        raise ValueError("coclr_amd: data must be the flat uint8 tensor of jpeg.pack")


def _geometry(meta):
    _host_meta(meta)
    head = meta[:, :8]
    if not bool((head == head[0]).all()):
        raise ValueError("coclr_amd: the frames of one decode share size, components and sampling")
    width, H, W, ncomp, hs, vs = [int(v) for v in head[0, :6]]
    if width != meta.shape[1]:
        raise ValueError("coclr_amd: meta is %d words wide and says %d" % (meta.shape[1], width))
    ops.jpeg_workspace(H, W, ncomp, hs, vs)                               # refuses a geometry the kernels do not take
    return H, W, ncomp, hs, vs


def _cat(packs, who, one_geometry):
    """The body of cat and cat_ragged: each pack on its own is one `pack` wrote, and with `one_geometry` all agree."""
    packs = list(packs)
    if not packs:
        raise ValueError("coclr_amd: %s needs at least one pack" % who)
    geo = [_geometry(m) for _, m in packs]
    if one_geometry and any(g != geo[0] for g in geo):
        raise Unsupported("packs differ in size, components or sampling: %s" % sorted(set(geo)))
    width = max(m.shape[1] for _, m in packs)
    rows, offset = [], 0
    for data, m in packs:
        r = torch.zeros(m.shape[0], width, dtype=torch.int32)
        r[:, :m.shape[1]] = m
        r[:, 0] = width
        r[:, 8] += offset
        offset += data.numel()
        rows.append(r)
    if offset > 0x7fffffff:
        raise ValueError("coclr_amd: one decode takes up to 2 GiB of compressed bytes")
    return torch.cat([d for d, _ in packs]), torch.cat(rows)


def cat(packs):
    """The packs of a batch -> one (data, meta): the default collate cannot stack ragged bytes.  Byte offsets are
    shifted, and descriptors are padded to the widest pack (the one with the most restart segments)."""
    return _cat(packs, "cat", True)


def cat_ragged(packs):
    """`cat` for packs that DIFFER in size, components or sampling (videos that keep their own aspect ratio): byte
    offsets are shifted and descriptors padded to the widest pack as there, and every row keeps its own 8-word
    geometry head, which is what decode_ragged reads.  Packs of one geometry give exactly `cat`'s result."""
    return _cat(packs, "cat_ragged", False)


def _check_rows(data, meta, H, W, ncomp, hs, vs):
    """What the decode entry points check of every frame's row, said in words, before anything is uploaded.  The
    geometry is per frame, int64 (F,) tensors; where all frames share one, plain integers do (they broadcast)."""
    m = meta[:, 8:].to(torch.int64)
    n, width = data.numel(), m.shape[1]
    mcus = -(-W // (8 * hs)) * -(-H // (8 * vs))
    off, ln, ri, nseg = m[:, 0], m[:, 1], m[:, 2], m[:, 3]
    if bool(((off < 0) | (ln < 0) | (off + ln > n)).any()):
        raise ValueError("coclr_amd: a frame's bytes leave the buffer of %d bytes" % n)
    want = torch.where(ri > 0, -(-mcus // ri.clamp(min=1)), torch.ones_like(ri))
    if bool(((ri < 0) | (nseg != want) | (nseg > width - META_SEG)).any()):
        raise ValueError("coclr_amd: a frame's restart segments do not match its interval and its MCU count")
    seg = m[:, META_SEG:]
    live = torch.arange(seg.shape[1])[None, :] < nseg[:, None]
    prev = torch.cat([torch.zeros_like(seg[:, :1]), seg[:, :-1]], 1)
    if bool((live & ((seg < prev) | (seg > ln[:, None]))).any()):
        raise ValueError("coclr_amd: a restart segment's offset decreases or leaves its frame's bytes")
    q = m[:, META_QUANT:META_QUANT + 192]
    bad = (q < 0) | (q > 255)
    if bool(bad.any()) and bool((bad & (torch.arange(192) < 64 * torch.as_tensor(ncomp)[..., None])).any()):
        raise ValueError("coclr_amd: a quantiser outside 0..255")       # (in a component the frame has)


def check_meta(data, meta):
    """What coclr_jpeg_decode checks, said in words, before anything is uploaded."""
    geo = _geometry(meta)
    _flat_data(data)
    _check_rows(data, meta, *geo)
    return geo


def check_meta_ragged(data, meta):
    """check_meta for the rows of cat_ragged, each against its OWN geometry head -> int64 (F, 5): H, W, components,
    hs, vs per frame."""
    _host_meta(meta)
    _flat_data(data)
    head = meta[:, :8].to(torch.int64)
    if bool((head[:, 0] != meta.shape[1]).any()):
        raise ValueError("coclr_amd: meta is %d words wide and a row says otherwise" % meta.shape[1])
    if bool((head[:, 6:] != 0).any()):
        raise ValueError("coclr_amd: a row's geometry head is not one jpeg.pack wrote")
    geo = head[:, 1:6]
    for g in sorted(set(tuple(r) for r in geo.tolist())):
        ops.jpeg_workspace(*g)                           # refuses a geometry the kernels do not take
    _check_rows(data, meta, *geo.unbind(1))
    return geo.contiguous()


def split_policy(chunk_bytes=None):
    """The chunk size of a decode call: `chunk_bytes` if given, else COCLR_JPEG_SPLIT, else DEFAULT_SPLIT.  0 is the
    serial path; anything but 0 or 8..65536 is a ValueError."""
    what = "chunk_bytes"
    if chunk_bytes is None:
        text = os.environ.get("COCLR_JPEG_SPLIT")
        if text is None or text.strip() == "":
            return DEFAULT_SPLIT
        what = "COCLR_JPEG_SPLIT"
        try:
            chunk_bytes = int(text)
        except ValueError:
            raise ValueError("coclr_amd: COCLR_JPEG_SPLIT must be 0 or a chunk size in 8..65536, got %r" % text)
    try:
        whole = not isinstance(chunk_bytes, bool) and int(chunk_bytes) == chunk_bytes
    except (TypeError, ValueError):
        whole = False
    if not whole:
        raise ValueError("coclr_amd: %s must be an integer, got %r" % (what, chunk_bytes))
    chunk_bytes = int(chunk_bytes)
    if chunk_bytes != 0 and not 8 <= chunk_bytes <= 65536:
        raise ValueError("coclr_amd: %s must be 0 or a chunk size in 8..65536, got %d" % (what, chunk_bytes))
    return chunk_bytes


def decode(data, meta, out=None, device=None, max_stage_bytes=256 << 20, return_status=False, chunk_bytes=None):
    """(data, meta) of pack / cat -> (F, H, W, 3) uint8 on the device, the bytes PIL's convert('RGB') returns.
    A bad `meta` is refused on the host; the bytes are uploaded once; whole frames are decoded `max_stage_bytes` of
    intermediate storage (coefficients + sample planes) at a time.  `out`: a contiguous (F, H, W, 3) uint8 device
    tensor to fill (a view into a larger buffer will do).  The per-frame int32 status (0 = clean; 1: a bit pattern
    that is no Huffman code, 2: a run past the block -- a damaged file) is returned with return_status=True and
    kept in `decode.last_status` otherwise.  `chunk_bytes`: how frames without restart markers are entropy-decoded
    (module docstring): 0 one lane per frame, 8..65536 one lane per chunk of that many bytes, None the policy of
    COCLR_JPEG_SPLIT; the result does not depend on it."""
    chunk_bytes = split_policy(chunk_bytes)
    H, W, ncomp, hs, vs = check_meta(data, meta)
    F = meta.shape[0]
    if device is None:
        device = out.device if out is not None else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if out is None:
        out = torch.empty(F, H, W, 3, dtype=torch.uint8, device=device)
    elif tuple(out.shape) != (F, H, W, 3) or out.dtype != torch.uint8 or not out.is_contiguous() or not out.is_cuda:
        raise ValueError("coclr_amd: out must be a contiguous uint8 device tensor %s" % ((F, H, W, 3),))
    cb, pb = ops.jpeg_workspace(H, W, ncomp, hs, vs)
    per = max(1, min(F, int(max_stage_bytes) // (cb + pb)))
    host = meta[:, 8:].contiguous()
    d_data, d_meta = data.contiguous().to(device), host.to(device)
    coefs = torch.empty(per * cb // 2, dtype=torch.int16, device=device)
    planes = torch.empty(per * pb, dtype=torch.uint8, device=device)
    status = torch.empty(F, dtype=torch.int32, device=device)
    for k in range(0, F, per):
        e = min(F, k + per)
        ops.jpeg_decode(d_data, d_meta[k:e], host[k:e], H, W, ncomp, hs, vs, coefs, planes, out[k:e], status[k:e],
                        chunk_bytes=chunk_bytes)
    decode.last_status = status
    return (out, status) if return_status else out


decode.last_status = None


def ragged_plan(geo, max_stage_bytes):
    """Host tables of decode_ragged for frames of geometry `geo` (int64 (F, 5)): the output layout -- every frame in
    batch order, each starting 16-byte aligned -- and the stages: runs of whole frames whose workspace (coefficients
    + sample planes) stays within max_stage_bytes, one frame at least.  Returns (offset, total bytes, stages, blocks):
    a stage is (first frame, end frame, geom int64 (n, 8), prefix int64 (2, n + 1)), `blocks` the largest stage's."""
    F = geo.shape[0]
    g = geo.tolist()
    nblocks, rows, size = [], [], []
    for H, W, ncomp, hs, vs in g:
        mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
        nblocks.append(mx * my * (1 if ncomp == 1 else hs * vs + 2))
        rows.append(H * -(-W // 16))
        size.append(3 * H * W)
    offset, at = [], 0
    for n in size:
        offset.append(at)
        at = (at + n + 15) & ~15
    total = offset[-1] + size[-1]
    stages, k, most = [], 0, 1
    limit = max(1, int(max_stage_bytes))
    while k < F:
        e, used = k, 0
        while e < F and (e == k or used + nblocks[e] * 192 <= limit):
            used += nblocks[e] * 192
            e += 1
        geom = torch.zeros(e - k, ops.JR_FIELDS, dtype=torch.int64)
        prefix = torch.zeros(2, e - k + 1, dtype=torch.int64)
        geom[:, :5] = geo[k:e]
        nb = torch.tensor(nblocks[k:e], dtype=torch.int64)
        prefix[0, 1:] = nb.cumsum(0)
        prefix[1, 1:] = torch.tensor(rows[k:e], dtype=torch.int64).cumsum(0)
        geom[:, 5] = prefix[0, :-1]
        geom[:, 6] = torch.tensor(offset[k:e], dtype=torch.int64)
        most = max(most, int(prefix[0, -1]))
        stages.append((k, e, geom, prefix))
        k = e
    return torch.tensor(offset, dtype=torch.int64), total, stages, most


def decode_ragged(data, meta, device=None, max_stage_bytes=256 << 20, return_status=False, chunk_bytes=None):
    """(data, meta) of cat_ragged -> staging.RaggedFrames: every frame at its own size, the bytes PIL's convert('RGB')
    returns, in ONE flat device buffer in batch order -- what stage_train_clips_ragged and
    stage_classifier_clips_ragged take.  One call may mix sizes, gray and YCbCr and the three samplings; the stages
    are still one launch each for the whole batch (coclr_jpeg_decode_ragged).  A bad `meta` is refused on the host,
    row by row against the row's own geometry; status, `decode_ragged.last_status` and `chunk_bytes` as in `decode`.
    Whole frames are decoded `max_stage_bytes` of intermediate storage at a time; the result depends on neither."""
    from . import staging
    chunk_bytes = split_policy(chunk_bytes)
    geo = check_meta_ragged(data, meta)
    F = meta.shape[0]
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    offset, total, stages, blocks = ragged_plan(geo, max_stage_bytes)
    host = meta[:, 8:].contiguous()
    d_data, d_meta = data.contiguous().to(device), host.to(device)
    tables = torch.cat([t.reshape(-1) for _, _, geom, prefix in stages for t in (geom, prefix)])
    d_tables = tables.to(device)                                             # every stage's tables in one upload
    pixels = torch.empty((total + 15) & ~15, dtype=torch.uint8, device=device)
    coefs = torch.empty(blocks * 64, dtype=torch.int16, device=device)
    planes = torch.empty(blocks * 64, dtype=torch.uint8, device=device)
    status = torch.empty(F, dtype=torch.int32, device=device)
    at = 0
    for k, e, geom, prefix in stages:
        d_geom = d_tables[at:at + geom.numel()].view(geom.shape)
        at += geom.numel()
        d_prefix = d_tables[at:at + prefix.numel()].view(prefix.shape)
        at += prefix.numel()
        ops.jpeg_decode_ragged(d_data, d_meta[k:e], host[k:e], d_geom, geom, d_prefix, prefix, coefs, planes, pixels,
                               status[k:e], chunk_bytes=chunk_bytes)
    decode_ragged.last_status = status
    frames = staging.RaggedFrames(pixels, offset, geo[:, 0].to(torch.int32), geo[:, 1].to(torch.int32))
    return (frames, status) if return_status else frames


decode_ragged.last_status = None


def _window_mcus(geo, boxes):
    """window_mcus for int64 tables: geo (n, 5) H, W, components, hs, vs; boxes (n, 4) -> int64 (n, 4)."""
    H, W, ncomp, hs, vs = geo.unbind(1)
    x0, y0, w, h = boxes.unbind(1)

    def axis(p0, n, size, s):
        last = p0 + n - 1
        lo, hi = p0 // (8 * s), last // (8 * s)
        sub = (ncomp == 3) & (s == 2)
        clo = ((p0 >> 1) - 1).clamp(min=0) // 8
        chi = torch.minimum((size + 1) // 2 - 1, (last >> 1) + 1) // 8
        return torch.where(sub, torch.minimum(lo, clo), lo), torch.where(sub, torch.maximum(hi, chi), hi) + 1

    (mx0, mx1), (my0, my1) = axis(x0, w, W, hs), axis(y0, h, H, vs)
    return torch.stack([mx0, my0, mx1, my1], 1)


def window_mcus(H, W, ncomp, hs, vs, x0, y0, w, h):
    """The MCU rectangle (mx0, my0, mx1, my1), ends exclusive, that holds every sample the decoder reads for the pixel
    box (x0, y0, w, h) of a frame (csrc/jpeg_core.h: jc_window_init, which the entry point runs itself): the box's luma
    samples and, on an axis subsampled by 2, chroma columns or rows (p >> 1) - 1 .. (p >> 1) + 1 clamped to the plane."""
    return tuple(_window_mcus(torch.tensor([[H, W, ncomp, hs, vs]]), torch.tensor([[x0, y0, w, h]]))[0].tolist())


def _check_boxes(boxes, geo):
    """`boxes` of Store.decode / Store.plan against the selected frames' geometry -> int64 (n, 4) on the host."""
    n = geo.shape[0]
    try:
        boxes = torch.as_tensor(boxes)
    except (TypeError, ValueError, RuntimeError):
        raise ValueError("coclr_amd: boxes must be an integer (n, 4) tensor or sequence: x0, y0, w, h per frame")
    if boxes.is_floating_point() or boxes.is_complex() or boxes.dtype == torch.bool or tuple(boxes.shape) != (n, 4):
        raise ValueError("coclr_amd: boxes must be integers of shape (%d, 4): x0, y0, w, h per selected frame, got %s %s"
                         % (n, boxes.dtype, tuple(boxes.shape)))
    boxes = boxes.to("cpu", torch.int64).contiguous()
    x0, y0, w, h = boxes.unbind(1)
    if bool(((w < 1) | (h < 1)).any()):
        raise ValueError("coclr_amd: a box is at least 1 x 1")
    if bool(((x0 < 0) | (y0 < 0) | (x0 > geo[:, 1] - w) | (y0 > geo[:, 0] - h)).any()):
        raise ValueError("coclr_amd: a box leaves its frame")
    return boxes


def _store_policy(chunk_bytes):
    """A store's chunk size: `chunk_bytes` if given, else DEFAULT_STORE_CHUNK; 8..65536 (a store has no serial path)."""
    chunk_bytes = split_policy(DEFAULT_STORE_CHUNK if chunk_bytes is None else chunk_bytes)
    if chunk_bytes == 0:
        raise ValueError("coclr_amd: a store's chunk_bytes must be in 8..65536, got 0")
    return chunk_bytes


def _gather_tables(frames, slot, rec, lanes, records):
    """The placement of a gather (csrc/jpeg_core.h: JG_*): `frames` the m distinct frames as the plan names them (inside
    their store, or inside their shard), `rec` their records and `lanes` their entropy lanes, in the order they take in
    the arena; `slot` the plan entry of each of the n selected frames and `records` their records (a copy, rebased
    here) -> (plan, slot, records, arena bytes, arena rows)."""
    src, ln = rec[:, 0], rec[:, 1]
    words = torch.where(ln > 0, ((src + ln + 15) >> 4) - (src >> 4), torch.zeros_like(ln))
    dst = ((words.cumsum(0) - words) << 4) + (src & 15)
    nrows = torch.where(rec[:, 3] == 1, lanes, torch.zeros_like(ln))
    dstrow = nrows.cumsum(0) - nrows
    lanes = words + nrows
    plan = torch.stack([frames, src, ln, dst, rec[:, 6], nrows, dstrow, lanes.cumsum(0) - lanes], 1).contiguous()
    records[:, 0], records[:, 6] = dst[slot], dstrow[slot]
    return plan, slot.contiguous(), records, int(words.sum()) << 4, int(nrows.sum())


def _arena_views(self, nbytes, nrows):
    """The kept device arena of `self` (a Store or a ShardedStore), grown to hold `nbytes` and `nrows` -> its views."""
    # 16 bytes of room, as every store's bytes have; coclr_jpeg_store takes no store without a byte or a row
    self._arena = Store._grown(self._arena, (max(16, nbytes) + 16,), dtype=torch.uint8, device=self.device)
    self._arena_rows = Store._grown(self._arena_rows, (max(1, nrows), ops.JS_ROW_WORDS), dtype=torch.int32,
                                    device=self.device)
    return self._arena[:max(16, nbytes)], self._arena_rows[:max(1, nrows)]


def _decode_store(self, gathers, ids, boxes, max_stage_bytes):
    """The body of Store.decode and ShardedStore.decode -> (frames, status).  `gathers`: the selection's distinct
    frames are first copied to the device arena (self.gather_plan, self._gather) and decoded there as frames
    0 .. F-1; else the kernels read self._buffers() through the selection."""
    from . import staging
    window = None
    if boxes is None:
        sel, geo, offset, total, stages, blocks = self.plan(ids, max_stage_bytes)
    else:
        sel, geo, offset, total, stages, blocks, window = self.plan(ids, max_stage_bytes, boxes)
    F, device = sel.numel(), self.device
    gather, moved = None, []
    if gathers:                                                # the kernels see the arena's frames 0 .. F-1
        gather = self.gather_plan(sel)
        sel = torch.arange(F, dtype=torch.int64)
        moved = [gather[0].reshape(-1), gather[2].reshape(-1)] + [t.reshape(-1) for t in gather[5:]]
    tables = torch.cat([sel] + [t.reshape(-1) for _, _, geom, prefix in stages for t in (geom, prefix)] + moved +
                       ([] if window is None else [window.reshape(-1)]))
    d_tables = tables.to(device)                                             # the selection and every stage's tables
    d_sel = d_tables[:F]
    d_window = None if window is None else d_tables[tables.numel() - window.numel():].view(window.shape)
    pixels = torch.empty((total + 15) & ~15, dtype=torch.uint8, device=device)
    coefs = torch.empty(blocks * 64, dtype=torch.int16, device=device)
    planes = torch.empty(blocks * 64, dtype=torch.uint8, device=device)
    status = torch.empty(F, dtype=torch.int32, device=device)
    at = F
    if gather is None:
        store = self._buffers()
    else:
        tail = tables.numel() - (0 if window is None else window.numel())
        store = self._gather(gather, d_tables[tail - sum(t.numel() for t in moved):tail])
    for k, e, geom, prefix in stages:
        d_geom = d_tables[at:at + geom.numel()].view(geom.shape)
        at += geom.numel()
        d_prefix = d_tables[at:at + prefix.numel()].view(prefix.shape)
        at += prefix.numel()
        if window is None:
            ops.jpeg_decode_store(store, d_sel[k:e], sel[k:e], d_geom, geom, d_prefix, prefix, coefs, planes,
                                  pixels, status[k:e])
        else:
            ops.jpeg_decode_store_window(store, d_sel[k:e], sel[k:e], d_geom, geom, d_window[k:e], window[k:e],
                                         d_prefix, prefix, coefs, planes, pixels, status[k:e])
    if window is None:
        frames = staging.RaggedFrames(pixels, offset, geo[:, 0].to(torch.int32), geo[:, 1].to(torch.int32))
    else:
        frames = staging.RaggedFrames(pixels, offset, window[:, 3].to(torch.int32), window[:, 2].to(torch.int32))
    return frames, status


class Store:
    """A dataset's JPEG frames kept compressed on the device, parsed and validated once, decoded by frame index.

        store = jpeg.Store(capacity_bytes, capacity_frames)      # once, before the epochs
        first = store.add(jpeg.pack(raws))                       # per video; its frames are first .. first + len - 1
        frames = store.decode(ids)                               # per step: a staging.RaggedFrames, as decode_ragged's

    `add` takes what `pack` returns for one video (any geometry, gray or YCbCr, any sampling, with or without restart
    markers), refuses what `check_meta` refuses, uploads the bytes and records, for every chunk of `chunk_bytes` raw
    bytes of a frame without restart markers, the serial Huffman decoder's state at the chunk's start
    (coclr_jpeg_store_index: the rounds of the split decoder, run once).  `decode` then decodes every chunk in one
    pass from its recorded state; frames with restart markers keep a lane per segment.  Frames, `status` and
    `decode.last_status` are bit for bit `decode_ragged`'s on the same bytes, whatever `chunk_bytes` is.

    The buffers are allocated once and never grow: `capacity_bytes` of compressed bytes (may exceed 2 GiB; one frame
    may not), `capacity_frames` records of 64 bytes (device and host), 16 bytes of row per `chunk_bytes` of capacity,
    `capacity_table_sets` sets of quantisers and Huffman tables (3 KiB each, stored once per distinct set: cv2 and PIL
    write the same tables into every frame of a dataset) and `capacity_segments` restart-segment offsets (default
    64 per frame).  `chunk_bytes=None` is DEFAULT_STORE_CHUNK.

    A dataset larger than the device's memory: `bytes_on="host"` keeps the compressed bytes and the chunk rows in
    pinned host memory (the records, table sets and segment words, 64 bytes per frame, stay on the device).  `add`
    then indexes through a device scratch the size of the largest pack, and `decode` first copies the selection's
    DISTINCT frames to a device arena in one launch (coclr_jpeg_store_gather: a frame selected several times crosses
    the bus once) and decodes them there with the same kernels; the arena is kept and grows to the largest call.
    Ids, results, status and refusals are those of a device store holding the same packs.

    `save(path)` writes a built store as data (a JSON header and .npy arrays); `Store.load(path, ...)` reads one back
    as either kind, without parsing or indexing anything, and `add` carries on from there.
    A dataset that fits the devices of a NODE but not one of them is sharded: class ShardedStore.
    Not in scope: one host arena shared between ranks, shards on other nodes, re-balancing shards, a gather that
    skips the arena for local frames, gathering only the chunks a pixel box needs (whole frames cross the bus), decode
    kernels that read host memory themselves, and splitting inside the restart segments of frames with restart
    markers."""

    FORMAT_VERSION = 1
    _FILES = ("data", "frames", "tables", "segs", "rows", "geo", "lanes")

    def __init__(self, capacity_bytes, capacity_frames, chunk_bytes=None, device=None, capacity_table_sets=64,
                 capacity_segments=None, bytes_on="device"):
        if bytes_on not in ("device", "host"):
            raise ValueError("coclr_amd: bytes_on must be 'device' or 'host', got %r" % (bytes_on,))
        self.bytes_on = bytes_on
        self.chunk_bytes = _store_policy(chunk_bytes)
        capacity_bytes, capacity_frames = int(capacity_bytes), int(capacity_frames)
        capacity_segments = 64 * capacity_frames if capacity_segments is None else int(capacity_segments)
        if capacity_bytes < 1 or capacity_frames < 1 or capacity_table_sets < 1 or capacity_segments < 0:
            raise ValueError("coclr_amd: a store's capacities are positive")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.capacity_bytes, self.capacity_frames, self.capacity_segments = capacity_bytes, capacity_frames, \
            capacity_segments
        words = ops.JS_TABLE_PAD + int(capacity_table_sets) * ops.JS_TABLE_WORDS
        rows = capacity_bytes // self.chunk_bytes + capacity_frames              # a frame has len // chunk + 1 at most
        self._host = (torch.zeros(capacity_frames, ops.JS_FIELDS, dtype=torch.int64),
                      torch.zeros(words, dtype=torch.int32), torch.zeros(max(1, capacity_segments), dtype=torch.int32))
        if bytes_on == "device":
            where = dict(device=self.device)
        else:                                                  # pinned, unless this is the CPU double of the tests
            where = dict(device="cpu", pin_memory=self.device.type == "cuda")
        # 16 bytes of room behind the bytes: coclr_jpeg_store_gather reads whole 16-byte words
        self._data = torch.empty(capacity_bytes + 16, dtype=torch.uint8, **where)[:capacity_bytes]
        self._dev = tuple(torch.zeros_like(t, device=self.device) for t in self._host)
        self._rows = torch.empty(rows, ops.JS_ROW_WORDS, dtype=torch.int32, **where)
        self._scratch = self._scratch_rows = self._arena = self._arena_rows = None     # a host store's, grown on demand
        self._sets = {}                                        # the 768 words' bytes -> table set
        self._geo = torch.zeros(capacity_frames, 5, dtype=torch.int64)    # host: H, W, components, hs, vs
        self._lanes = torch.zeros(capacity_frames, dtype=torch.int64)     # host: chunks, or restart segments
        self._frames = self._bytes = self._segs = self.chunk_rows = 0

    def __len__(self):
        return self._frames

    @property
    def nbytes(self):
        """Compressed bytes held (the write cursor)."""
        return self._bytes

    @property
    def table_sets(self):
        """Distinct sets of quantisers and Huffman tables held."""
        return len(self._sets)

    def frame_size(self, id):
        """(W, H) of frame `id`: what TrainTransform.draw takes."""
        id = int(id)
        if not 0 <= id < self._frames:
            raise ValueError("coclr_amd: frame %d of a store of %d" % (id, self._frames))
        return int(self._geo[id, 1]), int(self._geo[id, 0])

    def _advance_cursor(self, nbytes):
        """TEST ONLY: moves the write cursor by `nbytes` without writing, so that a test reaches byte offsets past
        2^31 without uploading that much."""
        if nbytes < 0 or self._bytes + nbytes > self.capacity_bytes:
            raise ValueError("coclr_amd: the cursor leaves the store")
        self._bytes += int(nbytes)

    def _buffers(self):
        """The arguments of ops.jpeg_store_desc."""
        frames, tables, segs = self._dev
        return (self._data, frames, self._host[0], self._frames, tables, self._host[1], len(self._sets), segs,
                self._host[2], self._segs, self._rows, self.chunk_bytes)

    def add(self, pack):
        """One video's (data, meta) of `pack` -> the id of its first frame; ids are consecutive in insertion order.
        ValueError, before anything is written: what check_meta refuses; more bytes, frames, table sets or
        restart segments than the store was made for."""
        data, meta = pack
        H, W, ncomp, hs, vs = check_meta(data, meta)
        F, n = meta.shape[0], data.numel()
        m = meta[:, 8:].to(torch.int64)
        ln, nseg = m[:, 1], m[:, 3]
        lanes = torch.where(nseg == 1, (-(-ln // self.chunk_bytes)).clamp(min=1), nseg)
        keys = [meta[f, 8 + META_QUANT:8 + META_SEG].numpy().tobytes() for f in range(F)]
        fresh = list(dict.fromkeys(k for k in keys if k not in self._sets))
        nsegs = int(nseg[nseg > 1].sum())
        host_frames, host_tables, host_segs = self._host
        for have, more, room, what in ((self._bytes, n, self.capacity_bytes, "bytes"),
                                       (self._frames, F, self.capacity_frames, "frames"),
                                       (len(self._sets), len(fresh), (host_tables.numel() - ops.JS_TABLE_PAD) //
                                        ops.JS_TABLE_WORDS, "table sets"),
                                       (self._segs, nsegs, self.capacity_segments, "restart segments")):
            if have + more > room:
                raise ValueError("coclr_amd: the store holds %d of %d %s and the pack brings %d" %
                                 (have, room, what, more))
        f0, s0 = self._frames, len(self._sets)
        for k in fresh:
            at = ops.JS_TABLE_PAD + len(self._sets) * ops.JS_TABLE_WORDS
            host_tables[at:at + ops.JS_TABLE_WORDS] = torch.frombuffer(bytearray(k), dtype=torch.int32)
            self._sets[k] = len(self._sets)
        rec = torch.zeros(F, ops.JS_FIELDS, dtype=torch.int64)
        rec[:, 0] = self._bytes + m[:, 0]
        rec[:, 1], rec[:, 2], rec[:, 3] = ln, m[:, 2], nseg
        rec[:, 4] = torch.tensor([self._sets[k] for k in keys], dtype=torch.int64)
        multi = nseg > 1
        rec[:, 5] = self._segs + torch.cumsum(torch.where(multi, nseg, 0), 0) - torch.where(multi, nseg, 0)
        rec[:, 6] = self.chunk_rows + torch.cumsum(torch.where(multi, 0, lanes), 0) - torch.where(multi, 0, lanes)
        rec[:, 7] = H | W << 16 | ncomp << 32 | hs << 36 | vs << 40
        host_frames[f0:f0 + F] = rec
        if nsegs:
            live = torch.arange(m.shape[1] - META_SEG)[None, :] < torch.where(multi, nseg, 0)[:, None]
            host_segs[self._segs:self._segs + nsegs] = m[:, META_SEG:][live].to(torch.int32)
        self._geo[f0:f0 + F] = torch.tensor([H, W, ncomp, hs, vs], dtype=torch.int64)
        self._lanes[f0:f0 + F] = lanes
        frames, tables, segs = self._dev
        self._data[self._bytes:self._bytes + n].copy_(data)
        frames[f0:f0 + F].copy_(rec)
        if fresh:
            a = ops.JS_TABLE_PAD + s0 * ops.JS_TABLE_WORDS
            tables[a:a + len(fresh) * ops.JS_TABLE_WORDS].copy_(host_tables[a:a + len(fresh) * ops.JS_TABLE_WORDS])
        if nsegs:
            segs[self._segs:self._segs + nsegs].copy_(host_segs[self._segs:self._segs + nsegs])
        was = self._frames, self._bytes, self._segs, self.chunk_rows
        self._frames, self._bytes, self._segs = f0 + F, self._bytes + n, self._segs + nsegs
        self.chunk_rows += int(lanes[~multi].sum())
        try:
            if self.bytes_on == "host":
                self._index_through_scratch(data, rec, was)
            else:
                ops.jpeg_store_index(self._buffers(), f0, f0 + F)
        except Exception:                                      # refused by the entry point: the frames are not kept
            self._frames, self._bytes, self._segs, self.chunk_rows = was
            for k in fresh:
                del self._sets[k]
            raise
        return f0

    @staticmethod
    def _grown(buf, shape, **where):
        """`buf` if it holds `shape` (its first dimension counts), else a new buffer half as large again."""
        if buf is not None and buf.shape[0] >= shape[0]:
            return buf
        return torch.empty((shape[0] + shape[0] // 2 + 16,) + tuple(shape[1:]), **where)

    def _index_through_scratch(self, data, rec, was):
        """A host store's indexing: the new pack's bytes go to a device scratch, coclr_jpeg_store_index runs on a store
        view of the pack alone -- its records rebased to the scratch, the tables and segment words the store's own --
        and the rows come back into the host rows.  A row is relative to its chunk, so these are the device store's."""
        _, bytes0, _, rows0 = was
        n, F, nrows = data.numel(), rec.shape[0], self.chunk_rows - rows0
        self._scratch = self._grown(self._scratch, (n + 16,), dtype=torch.uint8, device=self.device)
        self._scratch_rows = self._grown(self._scratch_rows, (max(1, nrows), ops.JS_ROW_WORDS), dtype=torch.int32,
                                         device=self.device)
        local = rec.clone()
        local[:, 0] -= bytes0
        local[:, 6] -= rows0
        self._scratch[:n].copy_(data)
        _, tables, segs = self._dev
        ops.jpeg_store_index((self._scratch[:max(1, n)], local.to(self.device), local, F, tables, self._host[1],
                              len(self._sets), segs, self._host[2], self._segs, self._scratch_rows, self.chunk_bytes),
                             0, F)
        if nrows:
            self._rows[rows0:rows0 + nrows].copy_(self._scratch_rows[:nrows])

    def gather_plan(self, sel):
        """The host tables of coclr_jpeg_store_gather for the selection `sel` (int64 (n,), inside the store) -> (plan
        int64 (m, 8), slot int64 (n,), records int64 (n, 8), arena bytes, arena rows): the m DISTINCT frames in store
        order with their places in the arena (csrc/jpeg_core.h: JG_*), the plan entry of every selected frame, and the
        selected frames' records rebased to the arena.  Frame j's first arena byte is congruent to its first store
        byte mod 16 and its hull of whole 16-byte words starts where the one before ends; rows are consecutive."""
        frames, slot = torch.unique(sel, return_inverse=True)
        return _gather_tables(frames, slot, self._host[0][frames], self._lanes[frames], self._host[0][sel])

    def _gather(self, gather, d_tables):
        """Copies the planned frames to the device arena, one launch -> the arguments of ops.jpeg_store_desc for the
        arena as a store: data and rows the arena's, frames the rebased records, tables and segment words this
        store's own.  `d_tables`: the plan and the records on the device, one after the other."""
        plan, slot, records, nbytes, nrows = gather
        arena, arena_rows = _arena_views(self, nbytes, nrows)
        d_plan = d_tables[:plan.numel()].view(plan.shape)
        d_records = d_tables[plan.numel():].view(records.shape)
        ops.jpeg_store_gather(self._buffers(), d_plan, plan, slot, records, arena, arena_rows)
        _, tables, segs = self._dev
        return (arena, d_records, records, records.shape[0], tables, self._host[1], len(self._sets), segs, self._host[2],
                self._segs, arena_rows, self.chunk_bytes)

    def plan(self, ids, max_stage_bytes=256 << 20, boxes=None):
        """The host tables of `decode` for the selection `ids` -> (sel int64 (n,), geo int64 (n, 5), offset, total
        bytes, stages, blocks): ragged_plan's tables for those frames in that order, every stage's prefix with a
        third row, the entropy lanes (chunks, or restart segments) of all frames before each one.
        With `boxes` (x0, y0, w, h per selected frame) the tables are those of coclr_jpeg_decode_store_window, and the
        tuple has a seventh member, the window table int64 (n, 4): offset and total lay out the h x w boxes, a stage's
        geom names those offsets and its first two prefix rows count the box's MCU rectangle and row groups.  The
        stages themselves, the coefficient blocks and `blocks` are unchanged: the workspace stays full-frame."""
        sel = torch.as_tensor(ids).reshape(-1)
        if sel.numel() < 1 or sel.is_floating_point() or sel.is_complex() or sel.dtype == torch.bool:
            raise ValueError("coclr_amd: ids must be integers, one at least")
        sel = sel.to("cpu", torch.int64).contiguous()
        if bool(((sel < 0) | (sel >= self._frames)).any()):
            raise ValueError("coclr_amd: ids must lie in [0, %d)" % self._frames)
        geo = self._geo[sel]
        offset, total, stages, blocks = ragged_plan(geo, max_stage_bytes)
        lanes = self._lanes[sel]
        out = []
        for k, e, geom, prefix in stages:
            p = torch.zeros(3, e - k + 1, dtype=torch.int64)
            p[:2] = prefix
            p[2, 1:] = lanes[k:e].cumsum(0)
            out.append((k, e, geom, p))
        if boxes is None:
            return sel, geo, offset, total, out, blocks
        boxes = _check_boxes(boxes, geo)
        size = 3 * boxes[:, 2] * boxes[:, 3]
        step = (size + 15) & ~15
        offset = step.cumsum(0) - step
        total = int(offset[-1] + size[-1])
        rect = _window_mcus(geo, boxes)
        per_mcu = torch.where(geo[:, 2] == 1, 1, geo[:, 3] * geo[:, 4] + 2)
        nblocks = (rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1]) * per_mcu
        rows = boxes[:, 3] * ((boxes[:, 2] + 15) // 16)
        for k, e, geom, p in out:
            geom[:, 6] = offset[k:e]
            p[0, 1:] = nblocks[k:e].cumsum(0)
            p[1, 1:] = rows[k:e].cumsum(0)
        return sel, geo, offset, total, out, blocks, boxes

    def decode(self, ids, boxes=None, return_status=False, max_stage_bytes=256 << 20):
        """Frames `ids` (an integer tensor or sequence, in batch order, repeats allowed) -> staging.RaggedFrames, as
        decode_ragged returns for the same frames in that order.  Ids outside [0, len(store)) are a ValueError before
        any launch.  Whole frames are decoded `max_stage_bytes` of intermediate storage at a time; the result does
        not depend on it.  The per-frame status is returned with return_status=True and kept in `decode.last_status`.
        `boxes`: an integer (n, 4) tensor or sequence, x0, y0, w, h per selected frame; frame i of the result is then
        that h x w region alone, bit for bit `decode(ids).frame(i)[y0:y0 + h, x0:x0 + w]`, and only the chunks, restart
        segments, blocks and pixels it needs are decoded (coclr_jpeg_decode_store_window; staging.clip_frames makes
        ids and boxes from a batch's plans).  A box of a wrong shape or type, smaller than 1 x 1 or leaving its frame
        is a ValueError before any launch.  The status then reports damage met in what WAS decoded only; clean files
        give 0 either way.  The workspace, and so `max_stage_bytes`, still counts full frames."""
        frames, status = _decode_store(self, self.bytes_on == "host", ids, boxes, max_stage_bytes)
        Store.decode.last_status = status
        return (frames, status) if return_status else frames

    _SLICE = 64 << 20        # bytes moved at a time by save and load

    def _filled(self, table_sets=None):
        """name -> (buffer, filled length along its first dimension) of everything `save` writes."""
        sets = ops.JS_TABLE_PAD + (len(self._sets) if table_sets is None else table_sets) * ops.JS_TABLE_WORDS
        return {"data": (self._data, self._bytes), "frames": (self._host[0], self._frames),
                "tables": (self._host[1], sets), "segs": (self._host[2], self._segs),
                "rows": (self._rows, self.chunk_rows), "geo": (self._geo, self._frames),
                "lanes": (self._lanes, self._frames)}

    @staticmethod
    def _constants():
        return {"JS_FIELDS": ops.JS_FIELDS, "JS_TABLE_WORDS": ops.JS_TABLE_WORDS, "JS_TABLE_PAD": ops.JS_TABLE_PAD,
                "JS_ROW_WORDS": ops.JS_ROW_WORDS}

    def save(self, path):
        """Writes the store to the directory `path` (made if missing): header.json -- format version, chunk_bytes, the
        JS_* constants, the counts -- and the filled part of every buffer as <name>.npy.  Data only.  The bytes and
        rows are written in slices, from the host buffers of a host store and downloaded from a device store's."""
        import json
        os.makedirs(path, exist_ok=True)
        filled = self._filled()
        for name, (buf, n) in filled.items():
            out = np.lib.format.open_memmap(os.path.join(path, name + ".npy"), mode="w+",
                                            dtype=np.dtype(str(buf.dtype).split(".")[1]), shape=(n,) + tuple(buf.shape[1:]))
            step = max(1, self._SLICE // max(1, buf[0:1].numel() * buf.element_size()))
            for a in range(0, n, step):
                out[a:a + step] = buf[a:min(n, a + step)].cpu().numpy()
            out.flush()
            del out
        header = {"format": "coclr_amd.jpeg.Store", "version": self.FORMAT_VERSION, "chunk_bytes": self.chunk_bytes,
                  "constants": self._constants(), "frames": self._frames, "bytes": self._bytes, "segments": self._segs,
                  "rows": self.chunk_rows, "table_sets": len(self._sets)}
        with open(os.path.join(path, "header.json"), "w") as f:
            json.dump(header, f, indent=1)

    @classmethod
    def load(cls, path, device=None, bytes_on="device", capacity_bytes=None, capacity_frames=None,
             capacity_table_sets=None, capacity_segments=None):
        """A store `save` wrote -> a Store of either kind, whichever kind wrote it: nothing is parsed and nothing is
        indexed.  Capacities default to what the file holds (the segment capacity to the constructor's 64 per frame
        where that is more); larger ones let `add` carry on, ids continuing.  The arrays are read memory-mapped, a slice
        at a time.  ValueError, before any buffer is made: a header of another format version, JS_* constants that are
        not this library's, counts that disagree with the arrays' shapes, a truncated array, capacities below what
        the file holds.  What the arrays HOLD is not trusted: the entry points validate every record per call."""
        import json
        try:
            with open(os.path.join(path, "header.json")) as f:
                head = json.load(f)
        except (OSError, ValueError) as e:
            raise ValueError("coclr_amd: no readable store header in %s: %s" % (path, e))
        if not isinstance(head, dict) or head.get("format") != "coclr_amd.jpeg.Store" or \
                head.get("version") != cls.FORMAT_VERSION:
            raise ValueError("coclr_amd: %s is not a store of format version %d" % (path, cls.FORMAT_VERSION))
        if head.get("constants") != cls._constants():
            raise ValueError("coclr_amd: the store was written with other JS_* constants: %r" % (head.get("constants"),))
        try:
            counts = {k: head[k] for k in ("frames", "bytes", "segments", "rows", "table_sets")}
            chunk_bytes = _store_policy(head["chunk_bytes"])
        except KeyError as e:
            raise ValueError("coclr_amd: the store header lacks %s" % e)
        if any(isinstance(v, bool) or not isinstance(v, int) or v < 0 for v in counts.values()):
            raise ValueError("coclr_amd: the store header's counts must be non-negative integers: %r" % (counts,))
        nf, nb, ns, nr, nt = (counts[k] for k in ("frames", "bytes", "segments", "rows", "table_sets"))
        want = {"data": ((nb,), np.uint8), "frames": ((nf, ops.JS_FIELDS), np.int64),
                "tables": ((ops.JS_TABLE_PAD + nt * ops.JS_TABLE_WORDS,), np.int32), "segs": ((ns,), np.int32),
                "rows": ((nr, ops.JS_ROW_WORDS), np.int32), "geo": ((nf, 5), np.int64), "lanes": ((nf,), np.int64)}
        arrays = {}
        for name, (shape, dtype) in want.items():
            try:
                arrays[name] = np.load(os.path.join(path, name + ".npy"), mmap_mode="r", allow_pickle=False)
            except Exception as e:                             # missing, cut short, or no array at all
                raise ValueError("coclr_amd: %s.npy of the store cannot be read: %s" % (name, e))
            if arrays[name].shape != shape or arrays[name].dtype != dtype:
                raise ValueError("coclr_amd: %s.npy holds %s %s where the header's counts ask for %s %s" %
                                 (name, arrays[name].dtype, arrays[name].shape, np.dtype(dtype), shape))
        caps = {"capacity_bytes": max(1, nb) if capacity_bytes is None else int(capacity_bytes),
                "capacity_frames": max(1, nf) if capacity_frames is None else int(capacity_frames),
                "capacity_table_sets": max(1, nt) if capacity_table_sets is None else int(capacity_table_sets)}
        caps["capacity_segments"] = max(ns, 64 * caps["capacity_frames"]) if capacity_segments is None else \
            int(capacity_segments)
        for (what, cap), have in zip(caps.items(), (nb, nf, nt, ns)):
            if cap < have:
                raise ValueError("coclr_amd: %s=%d is below the %d the file holds" % (what, cap, have))
        if caps["capacity_bytes"] // chunk_bytes + caps["capacity_frames"] < nr:
            raise ValueError("coclr_amd: the file holds %d rows, more than its bytes and frames can have" % nr)
        store = cls(chunk_bytes=chunk_bytes, device=device, bytes_on=bytes_on, **caps)
        store._frames, store._bytes, store._segs, store.chunk_rows = nf, nb, ns, nr
        for name, (buf, n) in store._filled(nt).items():
            step = max(1, cls._SLICE // max(1, buf[0:1].numel() * buf.element_size()))
            for a in range(0, n, step):
                buf[a:min(n, a + step)].copy_(torch.from_numpy(np.array(arrays[name][a:a + step])))
        sets = store._host[1][ops.JS_TABLE_PAD:ops.JS_TABLE_PAD + nt * ops.JS_TABLE_WORDS]
        store._sets = {sets[i * ops.JS_TABLE_WORDS:(i + 1) * ops.JS_TABLE_WORDS].numpy().tobytes(): i
                       for i in range(nt)}
        for dev, host in zip(store._dev, store._host):
            dev.copy_(host)
        return store


Store.decode.last_status = None


class _Shard:
    """What a ShardedStore keeps of one shard: `data` and `rows`, the buffers a gather reads (a Store's own, device or
    pinned host, or a peer's device buffers mapped through hipIpc), and host copies of its books as they were when the
    shard was sealed: n frames, nbytes, records (n, 8), table words (sets * 768), segment words, geo (n, 5), lanes (n)."""

    def __init__(self, data, rows, nbytes, rec, tables, segs, geo, lanes):
        self.data, self.rows, self.nbytes, self.rec, self.tables, self.segs, self.geo, self.lanes = \
            data, rows, int(nbytes), rec, tables, segs, geo, lanes
        self.n = rec.shape[0]

    @classmethod
    def of(cls, store):
        n, sets = len(store), store.table_sets
        rec, tables, segs = store._host
        return cls(store._data, store._rows, store.nbytes, rec[:n].clone(),
                   tables[ops.JS_TABLE_PAD:ops.JS_TABLE_PAD + sets * ops.JS_TABLE_WORDS].clone(),
                   segs[:store._segs].clone(), store._geo[:n].clone(), store._lanes[:n].clone())

    def blobs(self):
        """The books as two flat tensors, int64 and int32, and what `from_blobs` needs to cut them."""
        return (torch.cat([self.rec.reshape(-1), self.geo.reshape(-1), self.lanes]),
                torch.cat([self.tables, self.segs]))

    @classmethod
    def from_blobs(cls, data, rows, nbytes, n, sets, nsegs, i64, i32):
        w = sets * ops.JS_TABLE_WORDS
        return cls(data, rows, nbytes, i64[:8 * n].view(n, ops.JS_FIELDS), i32[:w], i32[w:w + nsegs],
                   i64[8 * n:13 * n].view(n, 5), i64[13 * n:14 * n])


_NODE_GROUP = None


def _node_group():
    """The gloo side channel of ShardedStore.join: the world group if that is gloo, else a gloo group of all ranks
    (built once, as model.pretrain's host group is)."""
    global _NODE_GROUP
    import torch.distributed as dist
    if _NODE_GROUP is None:
        if os.environ.get("MASTER_ADDR", "") in ("127.0.0.1", "localhost", "::1"):
            os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")     # a container need not resolve its own host name
        _NODE_GROUP = dist.new_group(backend="gloo") if dist.get_backend() != "gloo" else dist.group.WORLD
    return _NODE_GROUP


class ShardedStore:
    """One dataset's JPEG store in up to 8 shards, one per GPU of a node, decoded by GLOBAL frame index.

        sh = jpeg.ShardedStore([a, b, c])            # the shards are Stores of this process, device or host kind
        sh = jpeg.ShardedStore.join(store, group)    # collective: this rank's device Store becomes shard `rank`
        frames = sh.decode(ids)                      # Store.decode's contract, bit for bit

    Every rank of a data-parallel job draws from the whole dataset, so without sharding every rank holds every frame.
    Here each rank holds 1/W of the compressed bytes in its HBM and maps its peers' buffers through hipIpc; `decode`
    copies the selection's DISTINCT frames -- local ones included: one path, and a local copy runs at HBM speed -- from
    whichever shard holds them into a device arena in ONE launch (coclr_jpeg_store_gather_shards, 16 bytes per lane)
    and decodes them there with Store's kernels.  Frames, status, `decode.last_status`, refusals, boxes and
    `max_stage_bytes` staging are those of one Store that was given the same packs in global order.

    Ids: a global id is bases[s] + the frame's id inside shard s, `bases` the exclusive running sum of the shards'
    lengths in shard order; a one-shard ShardedStore has its Store's ids.  A shard may be empty.

    Sealing: the shards' books are copied when the ShardedStore is made and are immutable from then on -- `add` is a
    ValueError here; a Store passed in is not modified and stays usable on its own, but what is added to it later is
    not seen here.  The union of the shards' table sets, de-duplicated by their 768 words, is one device array; the
    shards' restart-segment words, concatenated, another; every record's set index and first segment word are remapped
    on the sealed host copy.  Shards that differ in chunk_bytes or device, and more than 8, are refused.
    Replicated on EVERY rank: 112 bytes of host memory per frame of the WHOLE dataset (record 64, geo 40, lanes 8), and
    on the device 4 bytes per restart segment and 3 KiB per distinct table set.  The compressed bytes and the chunk
    rows are not replicated.

    Lifetime, the one rule of `join`: a rank must not free its store, or leave, while a peer can still launch a gather
    on its buffers.  `close()` is the collective that ends that: every rank waits for its own device, drops its
    mappings and meets the others at a barrier; after it the Store is the rank's own again.
    The cross-GPU path has run as two processes on ONE device only (unmeasured: no multi-GPU node).
    Not in scope: shards on other nodes, re-balancing shards, a gather that skips the arena for local frames, one host
    arena shared between ranks."""

    MAX_SHARDS = ops.JG_MAX_SHARDS

    def __init__(self, shards):
        shards = list(shards)
        if not 1 <= len(shards) <= self.MAX_SHARDS or not all(isinstance(s, Store) for s in shards):
            raise ValueError("coclr_amd: a ShardedStore takes 1..%d Stores, got %d" % (self.MAX_SHARDS, len(shards)))
        if len({s.chunk_bytes for s in shards}) != 1 or len({s.device for s in shards}) != 1:
            raise ValueError("coclr_amd: the shards of a store share one chunk_bytes and one device, got %s on %s" %
                             ([s.chunk_bytes for s in shards], [str(s.device) for s in shards]))
        self._group = None
        self._seal([_Shard.of(s) for s in shards], shards[0].chunk_bytes, shards[0].device)

    def _seal(self, parts, chunk_bytes, device):
        self.chunk_bytes, self.device, self._parts = int(chunk_bytes), device, parts
        W, T = ops.JS_TABLE_WORDS, ops.JS_TABLE_PAD
        counts = torch.tensor([p.n for p in parts], dtype=torch.int64)
        self._ends = counts.cumsum(0)
        self._bases = self._ends - counts
        self._frames, self._bytes = int(counts.sum()), sum(p.nbytes for p in parts)
        self._sets, words, seg0 = {}, [], 0
        rec = torch.cat([p.rec for p in parts]).clone()
        for s, p in enumerate(parts):
            lo, hi = int(self._bases[s]), int(self._ends[s])
            remap = torch.zeros(max(1, p.tables.numel() // W), dtype=torch.int64)
            for i in range(p.tables.numel() // W):
                key = p.tables[i * W:(i + 1) * W].numpy().tobytes()
                if key not in self._sets:
                    self._sets[key] = len(self._sets)
                    words.append(p.tables[i * W:(i + 1) * W])
                remap[i] = self._sets[key]
            if bool(((p.rec[:, 4] < 0) | (p.rec[:, 4] >= p.tables.numel() // W)).any()):
                raise ValueError("coclr_amd: a record of shard %d names a table set the shard does not hold" % s)
            rec[lo:hi, 4] = remap[p.rec[:, 4]]
            rec[lo:hi, 5] += seg0
            seg0 += p.segs.numel()
        self._segs = seg0
        tables = torch.cat([torch.zeros(T, dtype=torch.int32)] + words)
        segs = torch.cat([p.segs for p in parts] + [torch.zeros(0 if seg0 else 1, dtype=torch.int32)])
        self._host = (rec, tables, segs)                                     # sealed: records, table words, segment words
        self._dev_tables, self._dev_segs = tables.to(device), segs.to(device)
        self._geo = torch.cat([p.geo for p in parts])
        self._lanes = torch.cat([p.lanes for p in parts])
        self._arena = self._arena_rows = None
        self._sources = [(p.data, p.rows, rec[int(self._bases[s]):int(self._ends[s])], p.n, tables, len(self._sets),
                          segs, seg0, self.chunk_bytes) for s, p in enumerate(parts)]

    @classmethod
    def join(cls, store, group=None):
        """COLLECTIVE over `group`, a gloo group of the ranks of ONE node (default: the world as a gloo group): this
        rank's device Store becomes shard `rank` of the store every rank gets back.  Every rank synchronises its
        device and exports its bytes and rows through hipIpc (torch's IPC tensor sharing carries the handles over the
        host channel); sizes travel first, then each rank's books as two flat tensors -- no per-frame pickling.  The
        outcome is the same on every rank: if any rank could not export or map, every rank raises the same
        RuntimeError and none is sharded.  ValueError: a `bytes_on="host"` store (pinned memory is not exported; that
        kind is legal in the in-process form), more than 8 ranks, ranks that differ in chunk_bytes."""
        import torch.distributed as dist
        from torch.multiprocessing.reductions import reduce_tensor
        if not isinstance(store, Store) or store.bytes_on != "device":
            raise ValueError("coclr_amd: ShardedStore.join takes this rank's device Store; a bytes_on='host' store "
                             "cannot be shared between processes")
        group = _node_group() if group is None else group
        world, rank = dist.get_world_size(group), dist.get_rank(group)
        if store.device.type == "cuda":
            torch.cuda.synchronize(store.device)
        mine, handles, err = _Shard.of(store), None, None
        try:
            handles = [reduce_tensor(store._data), reduce_tensor(store._rows)]
        except Exception as e:                                 # hipIpcGetMemHandle refused: still take part
            err = e
        i64, i32 = mine.blobs()
        head = torch.tensor([err is None, mine.n, mine.nbytes, mine.tables.numel() // ops.JS_TABLE_WORDS,
                             mine.segs.numel(), store.chunk_bytes, store._data.numel(), store._rows.shape[0]],
                            dtype=torch.int64)
        heads = [torch.zeros_like(head) for _ in range(world)]
        dist.all_gather(heads, head, group=group)                            # sizes first
        heads = torch.stack(heads)
        if world > cls.MAX_SHARDS or len(set(heads[:, 5].tolist())) != 1:
            raise ValueError("coclr_amd: ShardedStore.join takes 1..%d ranks of one chunk_bytes, got %d ranks with %s" %
                             (cls.MAX_SHARDS, world, heads[:, 5].tolist()))
        objs, parts, mapped = [None] * world, [], []
        dist.all_gather_object(objs, handles, group=group)
        for r in range(world):                                               # the books, rank by rank
            _, n, nbytes, sets, nsegs = heads[r, :5].tolist()
            a = i64 if r == rank else torch.empty(14 * n, dtype=torch.int64)
            b = i32 if r == rank else torch.empty(sets * ops.JS_TABLE_WORDS + nsegs, dtype=torch.int32)
            for t in (a, b):
                if t.numel():
                    dist.broadcast(t, src=dist.get_global_rank(group, r), group=group)
            parts.append((nbytes, n, sets, nsegs, a, b))
        try:
            if err is None and (not bool(heads[:, 0].all()) or any(o is None for o in objs)):
                raise RuntimeError("a peer could not export its buffers")
            for r in range(world if err is None else 0):
                if r == rank:
                    data, rows = store._data, store._rows
                else:
                    data, rows = [fn(*args) for fn, args in objs[r]]
                    mapped.extend([data, rows])
                    if data.dtype != torch.uint8 or data.numel() != int(heads[r, 6]) or rows.dtype != torch.int32 or \
                            tuple(rows.shape) != (int(heads[r, 7]), ops.JS_ROW_WORDS):
                        raise RuntimeError("rank %d's mapped buffers are not what it announced" % r)
                    for t in (data, rows):
                        if t.device != store.device:
                            t.reshape(-1)[:1].to(store.device)               # makes torch enable peer access to it
                parts[r] = _Shard.from_blobs(data, rows, *parts[r])
        except Exception as e:                                 # hipIpc across devices / processes refused here
            err = e
        ok = torch.tensor([0 if err is not None else 1], dtype=torch.int32)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN, group=group)               # agree, as pretrain._peer_stage does
        if int(ok) == 0:
            del mapped, parts
            raise RuntimeError("coclr_amd: ShardedStore.join: a rank could not export or map a shard's buffers "
                               "through hipIpc; no rank is sharded") from err
        self = cls.__new__(cls)
        self._group, self._mapped, self._own = group, mapped, store          # the mapped tensors are kept alive
        self._seal(parts, store.chunk_bytes, store.device)
        return self

    def close(self):
        """Drops the peers' mappings; after it `decode` is a ValueError.  For a joined store a COLLECTIVE: every rank
        waits for its own device (its gathers on its peers' buffers are done), drops its mappings, and leaves through
        a barrier -- so that no rank frees its store, or exits, while a peer can still launch a gather on it."""
        if self._parts is None:
            return
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        self._parts = self._sources = self._arena = self._arena_rows = None
        if self._group is not None:
            import torch.distributed as dist
            self._mapped = self._own = None
            dist.barrier(group=self._group)

    def __len__(self):
        return self._frames

    @property
    def nbytes(self):
        """Compressed bytes held by all shards."""
        return self._bytes

    @property
    def table_sets(self):
        """Distinct sets of quantisers and Huffman tables in the union."""
        return len(self._sets)

    @property
    def bases(self):
        """int64 (shards,): the global id of every shard's frame 0."""
        return self._bases.clone()

    def shard_of(self, ids):
        """The shard of every global id (int64, the shape of `ids`); ids outside [0, len) are a ValueError."""
        ids = torch.as_tensor(ids).to("cpu", torch.int64)
        if bool(((ids < 0) | (ids >= self._frames)).any()):
            raise ValueError("coclr_amd: ids must lie in [0, %d)" % self._frames)
        return torch.searchsorted(self._ends, ids.contiguous(), right=True)

    frame_size = Store.frame_size
    plan = Store.plan                                      # on the global geo and lanes

    def add(self, pack):
        raise ValueError("coclr_amd: a ShardedStore is sealed; add to a Store before it becomes a shard")

    def gather_plan(self, sel):
        """Store.gather_plan for global ids -> its tuple and, sixth, the shard column int64 (m,): the m distinct frames
        ordered by (shard, frame) -- which is the order of their global ids -- with plan[:, 0] the frame's id INSIDE its
        shard, bytes and rows counted there, and the congruence held to the frame's first shard byte."""
        frames, slot = torch.unique(sel, return_inverse=True)
        shard = self.shard_of(frames)
        rec = self._host[0]
        return _gather_tables(frames - self._bases[shard], slot, rec[frames], self._lanes[frames], rec[sel]) + \
            (shard.contiguous(),)

    def _gather(self, gather, d_tables):
        """Store._gather over the shards; `d_tables`: plan, records and shard column on the device, in that order."""
        plan, slot, records, nbytes, nrows, shard = gather
        arena, arena_rows = _arena_views(self, nbytes, nrows)
        a, b = plan.numel(), plan.numel() + records.numel()
        d_plan, d_records = d_tables[:a].view(plan.shape), d_tables[a:b].view(records.shape)
        ops.jpeg_store_gather_shards(self._sources, d_plan, plan, d_tables[b:], shard, slot, records, arena, arena_rows)
        return (arena, d_records, records, records.shape[0], self._dev_tables, self._host[1], len(self._sets),
                self._dev_segs, self._host[2], self._segs, arena_rows, self.chunk_bytes)

    def decode(self, ids, boxes=None, return_status=False, max_stage_bytes=256 << 20):
        """Store.decode for global ids: the same plan, the shard gather, the same kernels on the arena."""
        if self._parts is None:
            raise ValueError("coclr_amd: the ShardedStore was closed")
        frames, status = _decode_store(self, True, ids, boxes, max_stage_bytes)
        ShardedStore.decode.last_status = Store.decode.last_status = status
        return (frames, status) if return_status else frames


ShardedStore.decode.last_status = None


def decode_frames(raws, out=None, device=None, max_stage_bytes=256 << 20, chunk_bytes=None):
    """pack followed by decode: JPEG files of one size and sampling -> (F, H, W, 3) uint8 on the device."""
    chunk_bytes = split_policy(chunk_bytes)
    data, meta = pack(raws)
    return decode(data, meta, out=out, device=device, max_stage_bytes=max_stage_bytes, chunk_bytes=chunk_bytes)
