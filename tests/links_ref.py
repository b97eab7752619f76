"""The yardstick of the native link-table reader (include/ldweaver_amd.h 13) in pure Python: split by the line rules, check the
number grammar, call float() per token.  Test infrastructure, not part of the package."""
import gzip
import re

import numpy as np

NUMBER = re.compile(rb"[+-]?(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]+)?\Z")
PLAIN_INT = re.compile(rb"[+-]?[0-9]+\Z")
SPECIAL = {b"NA": float("nan"), b"NaN": float("nan"), b"nan": float("nan"), b"Inf": float("inf"), b"inf": float("inf"),
           b"-Inf": float("-inf"), b"-inf": float("-inf")}
LINE_MAX = 1 << 20


class Refused(ValueError):
    """A file the reader refuses: 1-based physical line and column of the first fault (leftmost in the earliest bad line)."""
    def __init__(self, line, col, why):
        super().__init__(f"line {line}, column {col}: {why}")
        self.line, self.col, self.why = line, col, why


def read_bytes(path):
    raw = open(path, "rb").read()
    return gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw


def parse(data: bytes, ncols: int, sep: bytes):
    """(columns: list of float64 arrays, per-column "all plain integer literals" flags) of the table in ``data``."""
    rows, plain = [], [True] * ncols
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    for ln, line in enumerate(lines, 1):
        if len(line) > LINE_MAX:
            raise Refused(ln, 1, "line too long")
        if line.endswith(b"\r"):
            line = line[:-1]
        if not line:
            continue
        toks = line.split(sep)
        vals = []
        for c, tok in enumerate(toks[:ncols]):
            if tok in SPECIAL:
                vals.append(SPECIAL[tok])
                plain[c] = False
            elif NUMBER.match(tok):
                vals.append(float(tok))
                plain[c] = plain[c] and PLAIN_INT.match(tok) is not None
            else:
                raise Refused(ln, c + 1, "not a number")
        if len(toks) < ncols:
            raise Refused(ln, len(toks) + 1, "missing field")
        if len(toks) > ncols:
            raise Refused(ln, ncols + 1, "extra field")
        rows.append(vals)
    a = np.array(rows, dtype=np.float64).reshape(len(rows), ncols)
    return [np.ascontiguousarray(a[:, c]) for c in range(ncols)], (plain if rows else [False] * ncols)


def read(path, ncols: int, sep: str):
    return parse(read_bytes(path), ncols, sep.encode())


def frame(path, names, sep: str):
    """The frame the native reader's ``to="frame"`` gives: int64 where every token of a column is a plain integer literal."""
    import pandas as pd
    cols, plain = read(path, len(names), sep)
    return pd.DataFrame({n: (c.astype(np.int64) if p else c) for n, c, p in zip(names, cols, plain)}, columns=names)


def same_bits(a, b) -> bool:
    """Equal doubles bit for bit, any NaN equal to any NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))


# ---- corpora (seeded) ---------------------------------------------------------------------------------------------------------------------------

def writer_tokens(rng, n, fmt):
    """Corpus (a): ``fmt`` (the library's ldw_format_number) of random doubles with |x| in [1e-8, 1e15), and integers."""
    x = np.exp(rng.uniform(np.log(1e-8), np.log(1e15), n)) * rng.choice([-1.0, 1.0], n)
    x = x[(np.abs(x) >= 1e-8) & (np.abs(x) < 0.999e15)]
    toks = [fmt(float(v)) for v in x]
    toks += [str(int(v)) for v in rng.integers(-10**9, 10**9, n // 4)]
    return toks


def adversarial_tokens(rng, n):
    """Corpus (b): long mantissas, wide exponents, subnormals, halfway cases, the odd spellings and every special token."""
    toks = []
    for _ in range(n):
        x = float(np.ldexp(rng.random(), int(rng.integers(-1070, 1020)))) * (1 if rng.random() < .5 else -1)
        k = int(rng.integers(0, 6))
        if k == 0:
            m = "".join(str(d) for d in rng.integers(0, 10, int(rng.integers(16, 26))))
            p = int(rng.integers(0, len(m)))
            toks.append(m[:p] + "." + m[p:])
        elif k == 1:
            toks.append("%de%d" % (int(rng.integers(1, 10**9)), int(rng.integers(-320, 321))))
        elif k == 2:
            toks.append(repr(float(np.ldexp(rng.random(), -1074 + int(rng.integers(0, 52))))))     # subnormal
        elif k == 3:
            mant, e = ("%.16e" % x).split("e")                                                    # 17 digits, nudged by +-1 in the 17th and beyond
            toks.append(mant + ["49999999999", "5", "50000000001", "4999", "5000"][int(rng.integers(0, 5))] + "e" + e)
        elif k == 4:
            toks.append("0." + "0" * int(rng.integers(20, 60)) + str(int(rng.integers(1, 10**6))))  # long zero runs
        else:
            toks.append(repr(x))
    toks += ["-0", "1e+05", "1E5", ".5", "5.", "NA", "NaN", "nan", "Inf", "-Inf", "inf", "-inf", "1" + "0" * 40, "9007199254740993", "4.9e-324",
             "2.4703282292062327e-324", "2.4703282292062328e-324", "1e23", "0e999", "+7", "007", "1e-400", "1e400"]
    return toks


def write_table(path, toks, ncols, sep="\t", newline="\n", final_newline=True, gz=False):
    """``toks`` laid out row by row (padded with "1" to a whole row).  Returns the number of rows."""
    toks = list(toks) + ["1"] * (-len(toks) % ncols)
    rows = [sep.join(toks[i:i + ncols]) for i in range(0, len(toks), ncols)]
    data = (newline.join(rows) + (newline if final_newline else "")).encode()
    (gzip.open if gz else open)(path, "wb").write(data)
    return len(rows)
