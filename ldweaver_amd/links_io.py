"""Link tables read from their files on the device (include/ldweaver_amd.h 13): ``sr_links.tsv`` and ``lr_links.tsv`` of
``perform_MI_computation`` and SpydrPick's output, the inputs of the reference's readers (R/io_functions.R:32-66).  The file's bytes go to the
GPU in chunks and are parsed there; the values are the correctly rounded doubles of the text, as ``float()`` gives them."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib as L

SR_COLS = ["clust_c", "pos1", "pos2", "clust1", "clust2", "len", "MI", "srp_max", "ARACNE"]   # R/io_functions.R:63
LR_COLS = ["pos1", "pos2", "c1", "c2", "len", "MI"]                                            # R/io_functions.R:35
SPYDRPICK_COLS = {4: ["pos1", "pos2", "len", "MI"], 5: ["pos1", "pos2", "len", "ARACNE", "MI"]}   # R/io_functions.R:40-47
KINDS = ("sr", "lr", "spydrpick")
READERS = ("pandas", "native")


def check_reader(reader):
    if reader not in READERS:
        raise ValueError(f"reader must be one of {READERS}, got {reader!r}")
    return reader == "native"


def tsv_probe(path, sep: str = "\t"):
    """(fields of the first non-empty line, whether the file is gzip).  Host only."""
    n, gz = C.c_int32(0), C.c_int32(0)
    from .engine import fasta_check
    fasta_check(L.lib().ldw_tsv_probe(os.fsencode(path), ord(sep), C.byref(n), C.byref(gz)), path)
    return n.value, bool(gz.value)


def table_shape(path, kind: str):
    """(separator, column names) of a link file of ``kind``; a SpydrPick file is probed for its four or five columns."""
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS}, got {kind!r}")
    if kind == "sr":
        return "\t", SR_COLS
    if kind == "lr":
        return "\t", LR_COLS
    n, _ = tsv_probe(path, " ")
    if n == 0:
        return " ", SPYDRPICK_COLS[4]
    if n not in SPYDRPICK_COLS:
        raise ValueError(f"a SpydrPick file has 4 or 5 space-separated columns; {path} has {n}")
    return " ", SPYDRPICK_COLS[n]


def read_links_native(path, kind: str, engine=None, sr_dist=20000, to: str = "frame", chunk_bytes: int = 0):
    """A link file parsed on the device.  ``kind``: "sr" (sr_links.tsv, nine columns), "lr" (lr_links.tsv, six) or "spydrpick" (space
    separated, four or five); rows of the last two with len < sr_dist are dropped like ``read_LongRangeLinks`` drops them.
    ``to="frame"``: a pandas frame with the reference's column names — int64 where every cell of the column was a plain integer literal,
    float64 otherwise — equal to ``pd.read_csv(..., float_precision="round_trip")`` for every file both accept, with one limit: the device holds
    every cell as a double, so a plain-integer column with a value of 2^53 or more in magnitude (which pandas keeps as an exact int64) is refused
    with a ValueError instead of coming back rounded.
    ``to="device"``: a dict of float64 torch tensors on the engine's GPU (``engine`` is needed: with no row dropped they alias the engine's
    buffer and live until its next read)."""
    if to not in ("frame", "device"):
        raise ValueError(f'to must be "frame" or "device", got {to!r}')
    sep, names = table_shape(path, kind)
    if to == "device" and engine is None:
        raise ValueError('to="device" needs the engine that will hold the columns')
    from .engine import Engine
    own = engine is None
    eng = Engine(0) if own else engine
    try:
        rows, _slow, is_int = eng.tsv_read(path, sep, len(names), chunk_bytes)
        if to == "device":
            cols = dict(zip(names, eng.tsv_columns()))
            if kind != "sr" and rows:
                drops = cols["len"] < float(sr_dist)
                if bool(drops.any()):
                    keep = ~drops
                    cols = {k: v[keep] for k, v in cols.items()}
            return cols
        import pandas as pd
        data = {}
        for k, name in enumerate(names):
            v = eng.tsv_fetch(k, rows)
            if rows and is_int[k]:
                if not bool(np.all(np.abs(v) < 2.0 ** 53)):
                    raise ValueError(f"{path}: the integer column {name!r} holds a value of 2^53 or beyond, which a double cannot hold exactly")
                v = v.astype(np.int64)
            data[name] = v
        df = pd.DataFrame(data, columns=names)
    finally:
        if own:
            eng.close()
    if kind != "sr":
        drops = df["len"] < sr_dist
        if drops.any():
            df = df[~drops].reset_index(drop=True)
    return df
