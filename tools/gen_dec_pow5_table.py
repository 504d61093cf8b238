#!/usr/bin/env python3
"""Writes 3dgsconverter_amd/csrc/dec_pow5_table.h: floor(5^q normalised to 128 bits) for q = -342 ... 308, the table of the
decimal -> float64 certificate (csrc/dec_to_f64.h), with exact integer arithmetic.

    python tools/gen_dec_pow5_table.py

5^q lies in [m, m + 1) * 2^e5 with 2^127 <= m < 2^128 and e5 = floor(log2 5^q) - 127; for 0 <= q <= 55 m * 2^e5 is 5^q itself.
floor(log2 5^q) is (152170 * q) >> 16 over the whole range (checked here, and again by tests/test_ply_text_host.py against the
library's own entries)."""
import os

QMIN, QMAX, EXACT_MAX = -342, 308, 55


def entry(q: int):
    """-> (m, e5)"""
    if q >= 0:
        v = 5 ** q
        b = v.bit_length()
        return (v << (128 - b) if b <= 128 else v >> (b - 128)), b - 128
    d = 5 ** -q
    k = d.bit_length() + 127
    return (1 << k) // d, -k


def main():
    rows = []
    for q in range(QMIN, QMAX + 1):
        m, e5 = entry(q)
        assert (1 << 127) <= m < (1 << 128) and e5 == ((152170 * q) >> 16) - 127, q
        assert (q >= 0 and (5 ** q).bit_length() <= 128) == (0 <= q <= EXACT_MAX), q
        rows.append("    {0x%016xull, 0x%016xull}, /* %d */ \\" % (m >> 64, m & ((1 << 64) - 1), q))
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3dgsconverter_amd", "csrc", "dec_pow5_table.h")
    with open(out, "w") as f:
        f.write("// dec_pow5_table.h -- written by tools/gen_dec_pow5_table.py, not by hand: {high, low} words of floor(5^q normalised to\n"
                "// 128 bits) for q = GSX_DEC_QMIN ... GSX_DEC_QMAX; exact (5^q itself, shifted) for 0 <= q <= GSX_DEC_EXACT_QMAX\n"
                "#pragma once\n#define GSX_DEC_QMIN (%d)\n#define GSX_DEC_QMAX %d\n#define GSX_DEC_EXACT_QMAX %d\n#define GSX_DEC_POW5_ROWS \\\n"
                % (QMIN, QMAX, EXACT_MAX))
        f.write("\n".join(rows) + "\n\n")
    print(out, len(rows), "entries")


if __name__ == "__main__":
    main()
