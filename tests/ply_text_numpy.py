"""The ASCII PLY body's contract in plain Python and numpy ("ASCII PLY bodies"), used by the host tests, the GPU tests
and the golden generator: the oracle -- `line.split()`, `float()` and `int()` behind the grammar and range checks, the refusals
with element and 1-based line -- and a writer that turns token tables or structured arrays into ASCII files with chosen number
formats, separators and line ends.  The mapping to the readers' rows is ply_read_numpy.convert, unchanged."""
import re
from decimal import Decimal, getcontext

import numpy as np

import ply_read_numpy as pn

FLOAT_TOKEN = re.compile(rb"^[+-]?(([0-9]+(\.[0-9]*)?|\.[0-9]+)([eE][+-]?[0-9]+)?|nan|inf|infinity)$", re.I)
INT_TOKEN = re.compile(rb"^[+-]?[0-9]+$")
FORMATS = {"f4": "%.9g", "f8": "%.17g"}            # integers: %d


class Refused(ValueError):
    def __init__(self, element, line, why):
        super().__init__("element %r, line %d: %s" % (element, line, why))
        self.element, self.line, self.why = element, line, why


# ---------------------------------------------------------------------------------------------------------- the oracle

def value(token: bytes, typ: str):
    """one token as a property of numpy type `typ` -> a numpy scalar, or ValueError"""
    if typ in ("f4", "f8"):
        if not FLOAT_TOKEN.match(token):
            raise ValueError("no decimal number")
        v = np.float64(float(token))
        with np.errstate(all="ignore"):
            return v if typ == "f8" else v.astype(np.float32)        # rounded twice, as numpy's own float32(str) is
    if not INT_TOKEN.match(token):
        raise ValueError("no integer")
    v, info = int(token), np.iinfo(typ)
    if not info.min <= v <= info.max:
        raise ValueError("out of range")
    return np.dtype(typ).type(v)


def parse_element(lines, name, count, props):
    """the element's next `count` lines -> a little-endian structured array; lines: the file's remaining lines (bytes, no \\n)"""
    dt = np.dtype([(p, "<" + t if t[1] != "1" else t) for p, t in props])
    out = np.zeros(count, dt)
    for i in range(count):
        if i >= len(lines):
            raise Refused(name, i + 1, "the body ends")
        words = lines[i].split()              # bytes.split(): runs of 0x20 0x09 0x0a 0x0b 0x0c 0x0d
        if not words:
            raise Refused(name, i + 1, "blank")
        if words[0].startswith(b"#"):
            raise Refused(name, i + 1, "begins with '#'")
        if len(words) != len(props):
            raise Refused(name, i + 1, "%d values for %d properties" % (len(words), len(props)))
        for w, (p, t) in zip(words, props):
            try:
                out[p][i] = value(w, t)
            except ValueError as e:
                raise Refused(name, i + 1, "property %r: %r %s" % (p, w, e)) from None
    return out


def parse(path):
    """an ASCII PLY of scalar properties -> [(element name, structured array)] in header order"""
    with open(path, "rb") as f:
        raw = f.read()
    end = raw.index(b"\n", raw.index(b"end_header")) + 1
    elements = []
    for line in raw[:end].decode("ascii").splitlines():
        w = line.split()
        if w and w[0] == "format":
            assert w[1] == "ascii", line
        elif w and w[0] == "element":
            elements.append((w[1], int(w[2]), []))
        elif w and w[0] == "property":
            elements[-1][2].append((w[2], pn.TYPES[w[1]]))
    lines = raw[end:].split(b"\n")
    if lines and lines[-1] == b"":            # the file ended with its last line's newline
        lines.pop()
    out = []
    for name, count, props in elements:
        out.append((name, parse_element(lines, name, count, props)))
        lines = lines[count:]
    return out


class PlyData(pn.PlyData):
    """the stand-in for plyfile.PlyData on ASCII files (tests/devtools/make_golden_ply_text.py)"""

    @staticmethod
    def read(path):
        return PlyData(parse(path))


def read(path, dialect):
    """-> (rows, [(name, array)] of the other elements): the oracle's elements through the reference's statements"""
    elements = parse(path)
    if not any(n == "vertex" for n, _ in elements):
        raise ValueError("PLY file does not contain 'vertex' element")
    rows = pn.convert(next(d for n, d in elements if n == "vertex"), dialect)
    return rows, [(n, d) for n, d in elements if n != "vertex"]


# ---------------------------------------------------------------------------------------------------------- the writer

def tokens_of(arr, formats=None):
    """a structured array -> (props, [[token str per property] per row]); formats: {type str or field name: format}"""
    fm = dict(FORMATS, **(formats or {}))
    props = [(f, arr.dtype[f].str[1:]) for f in arr.dtype.names]
    cols = []
    for f, t in props:
        spec = fm.get(f, fm.get(t, "%d"))
        col = arr[f].tolist() if t[0] != "f" else [float(v) for v in arr[f].astype(np.float64)]
        cols.append([spec % v if isinstance(spec, str) else spec(v) for v in col])
    return props, [list(r) for r in zip(*cols)] if cols else []


def write_text(path, elements, sep=" ", eol="\n", lead="", trail="", last_newline=True):
    """elements: [(name, props, rows of tokens)] -> an ASCII PLY; sep / lead / trail: what stands between, before and behind the
    tokens of a line (strings, or functions of (row, column) / row); eol: the line end (\\n or \\r\\n)"""
    pick = lambda s, *a: s(*a) if callable(s) else s      # noqa: E731
    body = []
    for _, _, rows in elements:
        for r, toks in enumerate(rows):
            line = pick(lead, r)
            for c, tok in enumerate(toks):
                line += (pick(sep, r, c) if c else "") + tok
            body.append(line + pick(trail, r))
    text = eol.join(body) + (eol if body and last_newline else "")
    head = pn.header_text([(n, len(rows), props) for n, props, rows in elements], "ascii").decode("ascii")
    if eol != "\n":
        head = head.replace("\n", eol)
    with open(path, "wb") as f:
        f.write(head.encode("ascii") + text.encode("latin-1"))
    return path


def write_arrays(path, elements, formats=None, **kw):
    """elements: [(name, structured array)] -> an ASCII PLY (write_text's options)"""
    return write_text(path, [(n,) + tokens_of(a, formats) for n, a in elements], **kw)


# ---------------------------------------------------------------------------------------------------------- the hard set

def _plain(d: Decimal) -> str:
    return format(d, "f")


def midpoint_tokens(values, small):
    """per float64 in `values`: the exact decimal of the midpoint to its successor in the format `small` ("f8": the next double;
    "f4": the next float32 above a float32 value), a token just above it and one just below"""
    getcontext().prec = 1200
    out = []
    for x in values:
        if small == "f8":
            nxt = np.nextafter(np.float64(x), np.float64(np.inf))
        else:
            nxt = np.float64(np.nextafter(np.float32(x), np.float32(np.inf)))
        mid = (Decimal(float(x)) + Decimal(float(nxt))) / 2
        tiny = Decimal(10) ** (mid.adjusted() - 60)
        out += [_plain(mid), _plain(mid + tiny), _plain(mid - tiny)]
    return out


def hard_tokens():
    """float tokens where a parser goes wrong: float64 midpoints and their neighbours, float32 midpoints (where rounding twice
    shows), the ranges' ends, the grammar's corners, long mantissas, huge exponents"""
    rng = np.random.default_rng(7)
    d = rng.standard_normal(12) * np.float64(10.0) ** rng.integers(-8, 9, 12)
    toks = midpoint_tokens(list(d) + [1.0, 9007199254740992.0, 0.1, 1e22, 1e23, 8.5e-300, 1.7e308], "f8")
    f = (rng.standard_normal(12) * 100).astype(np.float32)
    toks += midpoint_tokens([float(v) for v in f] + [1.0, 16777216.0, 1e-45, 1.1754942e-38], "f4")
    toks += ["1.00000005960464477539062500001", "1.0000000596046448", "1.0000001788139343261718750001", "9007199254740993",
             "9007199254740992.5", "9007199254740993.0000000000000000001"]
    toks += ["1e-40", "1e-320", "1e39", "1e309", "-0", "-0.0", "+.5", "5.", "1E5", "nan", "-NaN", "Infinity", "+inf", "-INF", "-iNfIniTy",
             "0e999999999", "1e-999999999", "4.9e-324", "2.4703282292062327e-324", "2.4703282292062328e-324", "2.2250738585072011e-308",
             "2.2250738585072014e-308", "1.7976931348623157e308", "1.7976931348623158e308", "1.7976931348623159e308",
             "3.4028235677973366e38", "3.4028235677973367e38", "0.000", "-.0e5", "00012.5000", "1e+5", "1e-05", "5.e3"]
    toks += ["1234567890123456789012345", "0.1234567890123456789012345", "1" * 80, "0." + "0" * 40 + "7" * 40, "9" * 25 + "e-5",
             "1." + "0" * 70 + "1", "0.3" + "0" * 30]
    return toks


REFUSED_FLOAT_TOKENS = ["1_0", "0x10", "0x1p3", "1e", "e5", ".", "+", "--1", "1.2.3", "in", "infinit", "nane", "1e5.0", "١".encode("utf-8").decode("latin-1"),
                        "1,5", "1d5", "#1"]
REFUSED_INT_TOKENS = {"u1": ["2.0", "256", "-1", "1e2", "+", "0x1f"], "i1": ["128", "-129"], "u2": ["65536", "-1"], "i2": ["32768", "-32769"],
                      "u4": ["-1", "4294967296", "99999999999999999999999"], "i4": ["2147483648", "-2147483649", "1.0"]}
ACCEPTED_INT_TOKENS = {"u1": ["0", "255", "+7", "-0", "007"], "i1": ["-128", "127"], "u2": ["65535"], "i2": ["-32768", "32767"],
                       "u4": ["4294967295", "+0"], "i4": ["-2147483648", "2147483647"]}
