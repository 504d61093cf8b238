"""TEST INFRASTRUCTURE: the reference's ``KSplatFormat.read`` (gsconverter/formats/ksplat.py:29-317) restated in vectorised
numpy, and a builder of .ksplat files the reference's own writer cannot make (several sections, many partially filled buckets,
padding rows, mixed degrees, arbitrary row bytes).

``read`` is checked against the reference's recorded rows on every case of tests/golden/ksplat_read_ref.npz
(tests/test_ksplat_read_host.py), which licenses it as the checker at sizes the golden file cannot hold.  It runs on the host's
numpy, so its NaN bits are x86's, like the reference's.  The statements are the reference's; only the two Python-level loops
are replaced: the per-splat bucket list (:148-156) by np.repeat, the per-field scatter through a dict (:237-315) by column
assignments.
"""
import hashlib
import struct

import numpy as np

HEADER_BYTES, SECTION_BYTES = 4096, 1024
BASE_BEFORE = ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"]
BASE_AFTER = ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]
SECTION_KEYS = (("splatCount", "I", 0), ("maxSplatCount", "I", 4), ("bucketSize", "I", 8), ("bucketCount", "I", 12),
                ("bucketBlockSize", "f", 16), ("bucketStorageSizeBytes", "H", 20), ("compressionScaleRange", "I", 24),
                ("storageSizeBytes", "I", 28), ("fullBucketCount", "I", 32), ("partiallyFilledBucketCount", "I", 36),
                ("shDegree", "H", 40))


def sha(rows) -> bytes:
    return hashlib.sha256(np.ascontiguousarray(rows).view(np.uint8).tobytes()).digest()


def n_coeffs(degree: int) -> int:
    return 3 * ((degree + 1) ** 2 - 1)        # structures.py:36


def define_dtype(degree: int) -> np.dtype:
    """structures.py:23-59 with has_scal=False, has_rgb=False"""
    return np.dtype([(f, "f4") for f in BASE_BEFORE] + [("f_rest_%d" % i, "f4") for i in range(n_coeffs(degree))]
                    + [(f, "f4") for f in BASE_AFTER])


def sh_count_of(degree: int) -> int:
    return 9 if degree == 1 else (24 if degree == 2 else 0)     # :138-140


def row_bytes(level: int, degree: int) -> int:
    return (44 + 4 * sh_count_of(degree)) if level == 0 else 24 + (2 if level == 1 else 1) * sh_count_of(degree)


def raw_dtype(level: int, sh_count: int) -> np.dtype:
    """:161-195"""
    if level == 0:
        d = [("pos", "<f4", (3,)), ("scale", "<f4", (3,)), ("rot", "<f4", (4,)), ("color", "u1", (4,))]
        sh = "<f4"
    else:
        d = [("pos", "<u2", (3,)), ("scale", "<u2", (3,)), ("rot", "<u2", (4,)), ("color", "u1", (4,))]
        sh = "<f2" if level == 1 else "u1"
    if sh_count:
        d.append(("sh", sh, (sh_count,)))
    return np.dtype(d)


def parse(data: bytes):
    """:31-102 -> (metadata, payload offset)"""
    head = data[:HEADER_BYTES]
    u = lambda fmt, off, buf=head: struct.unpack_from(fmt, buf, off)[0]   # noqa: E731
    v_major, v_minor = head[0], head[1]
    level = u("H", 20)
    meta = {"v_major": v_major, "v_minor": v_minor, "splat_count": u("I", 16), "compression_level": level, "min_sh": u("f", 36),
            "max_sh": u("f", 40), "sections": []}
    pos = HEADER_BYTES
    for _ in range(u("I", 4)):
        sec = data[pos:pos + SECTION_BYTES]
        if not sec:
            break
        pos += len(sec)
        info = {k: u(fmt, off, sec) for k, fmt, off in SECTION_KEYS}
        if info["compressionScaleRange"] == 0 and level >= 1:
            info["compressionScaleRange"] = 32767
        meta["sections"].append(info)
    return meta, pos


def colour_tables():
    """:229-234, :24-27 on every byte -> (f_dc[256], opacity[256]) float32"""
    b = np.arange(256, dtype=np.uint8)
    rgba_f = b.astype(np.float32) / 255.0
    f_dc = (rgba_f - 0.5) / 0.28209479177387814
    alpha = np.clip(b.astype(np.float32) / 255.0, 1e-7, 1.0 - 1e-7)
    with np.errstate(all="ignore"):
        return f_dc, np.log(alpha / (1.0 - alpha))


def read(path: str):
    """-> (rows, metadata), or the reference's exception"""
    with open(path, "rb") as f:
        data = f.read()
    meta, off = parse(data)
    level = meta["compression_level"]
    payload = data[off:]
    off = 0
    f_dc_t, opa_t = colour_tables()
    parts = []
    for s in meta["sections"]:
        pfb = s["partiallyFilledBucketCount"]
        lengths = np.zeros(0, np.uint32)
        if pfb > 0:
            lengths = np.frombuffer(payload[off:off + pfb * 4], dtype=np.uint32)
            off += pfb * 4
        bc = s["bucketCount"]
        centres = []
        if bc > 0:
            centres = np.frombuffer(payload[off:off + bc * 12], dtype=np.float32).reshape(-1, 3)
            off += bc * 12
        n = s["splatCount"]
        shc = sh_count_of(s["shDegree"])
        rd = raw_dtype(level, shc)
        chunk = payload[off:off + n * rd.itemsize]
        off += s["maxSplatCount"] * rd.itemsize
        if level >= 1:
            fb = s["fullBucketCount"]
            if len(lengths) < pfb:
                lengths[len(lengths)]                                # :155's IndexError at the first missing length
            counts = np.concatenate([np.full(fb, s["bucketSize"], np.int64), lengths.astype(np.int64)])
            assign = np.repeat(np.arange(fb + pfb, dtype=np.int64), counts)[:n]
        raw = np.frombuffer(chunk, dtype=rd)
        with np.errstate(all="ignore"):
            if level == 0:
                pos, scales, rots = raw["pos"], raw["scale"], raw["rot"]
            else:
                b_idx = np.array(assign, dtype=np.int32)
                cen = centres[b_idx]
                sf = (s["bucketBlockSize"] / 2.0) / s["compressionScaleRange"]
                sr = s["compressionScaleRange"]
                pos = (raw["pos"].astype(np.float32) - sr) * sf + cen
                scales = raw["scale"].view(np.float16).astype(np.float32)
                rots = ((raw["rot"].astype(np.float32) - 32767.5) / 32767.5) * 1.41421356
            sh = None
            if shc:
                if level == 0:
                    sh = raw["sh"]
                elif level == 1:
                    sh = raw["sh"].astype(np.float32)
                else:
                    sh = (raw["sh"].astype(np.float32) - 128.0) / 128.0
        if len(pos) != len(raw):
            raise NotImplementedError("broadcast between %d rows and %d bucket assignments" % (len(raw), len(pos)))
        parts.append((pos, scales, rots, raw["color"], sh))
    degree = max(s["shDegree"] for s in meta["sections"]) if meta["sections"] else 3
    dtype = define_dtype(degree)
    out = np.zeros(sum(len(p[0]) for p in parts), dtype)
    at = 0
    for pos, scales, rots, colour, sh in parts:
        o = out[at:at + len(pos)]
        for k, ax in enumerate("xyz"):
            o[ax] = pos[:, k]
            o["scale_%d" % k] = scales[:, k]
            o["f_dc_%d" % k] = f_dc_t[colour[:, k]]
        for k in range(4):
            o["rot_%d" % k] = rots[:, k]
        o["opacity"] = opa_t[colour[:, 3]]
        if sh is not None:
            for k in range(min(sh.shape[1], n_coeffs(degree))):
                o["f_rest_%d" % k] = sh[:, k]
        at += len(pos)
    return out, meta


# ---------------------------------------------------------------- file builder

def section(level, degree, n, rng=None, rows=None, max_splats=None, bucket_size=256, block_size=5.0, scale_range=32767,
            full_buckets=None, partial=None, centres=None, bucket_count=None, header_degree=None):
    """One section: `rows` (n_max x row_bytes uint8; random bytes from `rng` if None), its buckets and header values.  By default
    the buckets are the reference's writer's: n // bucket_size full ones and at most one partially filled."""
    rb = row_bytes(level, degree)
    max_splats = n if max_splats is None else max_splats
    if rows is None:
        rows = rng.integers(0, 256, (max_splats, rb), dtype=np.uint8)
    rows = np.ascontiguousarray(rows, np.uint8).reshape(-1, rb) if rb else rows
    if full_buckets is None:
        full_buckets = n // bucket_size if partial is None else 0
    if partial is None:
        partial = [n % bucket_size] if n % bucket_size else []
    partial = np.asarray(partial, np.uint32)
    if bucket_count is None:
        bucket_count = full_buckets + len(partial)
    if centres is None:
        centres = (rng.standard_normal((bucket_count, 3)) * 10).astype(np.float32)
    return {"level": level, "degree": degree if header_degree is None else header_degree, "n": n, "max": max_splats, "rows": rows,
            "bucket_size": bucket_size, "block_size": block_size, "scale_range": scale_range, "full": full_buckets,
            "partial": partial, "centres": np.asarray(centres, np.float32).reshape(-1, 3), "bucket_count": bucket_count}


def build_file(path, level, sections, max_section_count=None, version=(0, 1), min_sh=-2.0, max_sh=2.0):
    """header, section headers, then per section: partial-bucket lengths | centres | rows (the layout :108-145 walks)"""
    head = bytearray(HEADER_BYTES)
    head[0], head[1] = version
    struct.pack_into("<IIIIH", head, 4, len(sections) if max_section_count is None else max_section_count, len(sections),
                     sum(s["max"] for s in sections), sum(s["n"] for s in sections), level)
    struct.pack_into("<ff", head, 36, min_sh, max_sh)
    out = [bytes(head)]
    for s in sections:
        sh = bytearray(SECTION_BYTES)
        struct.pack_into("<IIIIfH", sh, 0, s["n"], s["max"], s["bucket_size"], s["bucket_count"], s["block_size"], 12)
        struct.pack_into("<IIIIH", sh, 24, s["scale_range"], (4 * len(s["partial"]) + 12 * len(s["centres"]) + s["rows"].size) & 0xFFFFFFFF,
                         s["full"], len(s["partial"]), s["degree"])
        out.append(bytes(sh))
    for s in sections:
        out += [s["partial"].astype("<u4").tobytes(), s["centres"].astype("<f4").tobytes(), s["rows"].tobytes()]
    blob = b"".join(out)
    with open(path, "wb") as f:
        f.write(blob)
    return path


def random_file(path, level, degree, n, seed, bucket_size=256, block_size=5.0, partial=None, full_buckets=None):
    """a one-section file of random row bytes (every u16 / float16 / byte pattern turns up), for the large checks"""
    rng = np.random.default_rng(seed)
    return build_file(path, level, [section(level, degree, n, rng, bucket_size=bucket_size, block_size=block_size, partial=partial,
                                            full_buckets=full_buckets)])


def pattern_file(path, level, degree=2):
    """65 536 rows: row i holds the u16 pattern i in every u16 slot (position, scale, rotation, level-1 sh), byte i & 255 in every
    byte slot (colour, opacity, level-2 sh); at level 0 the float32 slots hold patterns spread over the exponent range"""
    n = 65536
    i = np.arange(n, dtype=np.uint32)
    raw = np.zeros(n, raw_dtype(level, sh_count_of(degree)))
    if level == 0:
        w = (i << np.uint32(16)) | (i * np.uint32(40503) & np.uint32(0xFFFF))
        for f in ("pos", "scale", "rot", "sh"):
            raw[f] = w.view(np.float32)[:, None]
    else:
        for f in ("pos", "scale", "rot"):
            raw[f] = i.astype(np.uint16)[:, None]
        raw["sh"] = (i.astype(np.uint16).view(np.float16) if level == 1 else (i & 255).astype(np.uint8))[:, None]
    raw["color"] = (i & 255).astype(np.uint8)[:, None]
    rng = np.random.default_rng(level)
    return build_file(path, level, [section(level, degree, n, rng, rows=raw.view(np.uint8).reshape(n, -1), bucket_size=100,
                                            block_size=0.37)])


# ---------------------------------------------------------------- the device entry point's contract, in numpy

def half_bits(h):
    """float16 patterns -> float32 bits as csrc/ksplat_read.hip's ksr_half spells them: the cast, a NaN's bits moved as they are"""
    h = np.asarray(h, np.uint16)
    out = h.view(np.float16).astype(np.float32).view(np.uint32).copy()
    nan = ((h & 0x7C00) == 0x7C00) & ((h & 0x03FF) != 0)
    w = h.astype(np.uint32)
    out[nan] = (((w & 0x8000) << 16) | 0x7F800000 | ((w & 0x03FF) << 13))[nan]
    return out


def position_bits(u16, sr, sf, centre):
    """`(f32(u16) - sr) * sf + centre` with the NaN bits spelled out as x86_nan does (sr, sf: np.float32)"""
    with np.errstate(all="ignore"):
        t2 = (u16.astype(np.float32) - sr) * sf
        r = t2 + centre
    out = r.view(np.uint32).copy()
    c_bits = np.broadcast_to(centre, r.shape).view(np.uint32) if centre.flags.c_contiguous else np.ascontiguousarray(centre).view(np.uint32)
    nan = np.isnan(r)
    fix = np.where(np.isnan(centre), c_bits | np.uint32(0x00400000),
                   np.float32(sf).view(np.uint32) | np.uint32(0x00400000) if np.isnan(sf) else np.uint32(0xFFC00000))
    out[nan] = fix[nan]
    return out


def decode_sections(body: bytes, level, sections, prefix, n_coeffs_out, n_rows, tables):
    """What gsx_ksplat_unpack_dev computes from its arguments (include/gsx_hip.h): -> uint32[n_rows, 17 + n_coeffs_out].  The
    host tests run formats/ksplat_reader.py's plan through this to check every offset, count and prefix sum it hands to the
    device against the reference's rows."""
    rw = 17 + n_coeffs_out
    out = np.full((n_rows, rw), 0xDEADBEEF, np.uint32)
    tail = 9 + n_coeffs_out
    tab = np.asarray(tables, np.float32).view(np.uint32)
    prefix = np.asarray(prefix, np.uint32)
    for s in sections:
        n = int(s.n_rows)
        if n == 0:
            continue
        rd = raw_dtype(level, s.sh_count)
        assert s.rows_offset + n * rd.itemsize <= len(body)
        raw = np.frombuffer(body, rd, n, s.rows_offset)
        o = out[s.out_row:s.out_row + n]
        assert (o == 0xDEADBEEF).all(), "rows written twice"
        o[:] = 0
        if level == 0:
            o[:, 0:3] = raw["pos"].view(np.uint32)
            o[:, tail + 1:tail + 4] = raw["scale"].view(np.uint32)
            o[:, tail + 4:tail + 8] = raw["rot"].view(np.uint32)
        else:
            i = np.arange(n, dtype=np.int64)
            ends = prefix[s.prefix_offset:s.prefix_offset + s.n_partial].astype(np.int64)
            b = np.where(i < s.full_rows, i // max(int(s.bucket_size), 1), int(s.n_full) + np.searchsorted(ends, i, side="right"))
            assert b.max() < s.n_buckets and s.centres_offset + 12 * s.n_buckets <= len(body)
            cen = np.frombuffer(body, "<f4", 3 * int(s.n_buckets), s.centres_offset).reshape(-1, 3)[b]
            o[:, 0:3] = position_bits(raw["pos"], np.float32(s.scale_range), np.float32(s.scale_factor), np.ascontiguousarray(cen))
            o[:, tail + 1:tail + 4] = half_bits(raw["scale"])
            with np.errstate(all="ignore"):
                rot = ((raw["rot"].astype(np.float32) - np.float32(32767.5)) / np.float32(32767.5)) * np.float32(1.41421356)
            o[:, tail + 4:tail + 8] = rot.view(np.uint32)
        o[:, 6:9] = tab[raw["color"][:, :3]]
        o[:, tail] = tab[256 + raw["color"][:, 3].astype(np.int64)]
        if s.sh_count:
            if level == 0:
                sh = raw["sh"].view(np.uint32)
            elif level == 1:
                sh = half_bits(raw["sh"].view(np.uint16))
            else:
                sh = ((raw["sh"].astype(np.float32) - np.float32(128)) * np.float32(0.0078125)).view(np.uint32)
            o[:, 9:9 + s.sh_count] = sh
    assert not (out == 0xDEADBEEF).all(axis=1).any(), "rows not written"
    return out
