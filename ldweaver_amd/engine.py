"""Thin object wrapper over the C ABI: one Engine = one ldw_ctx on one GPU."""
from __future__ import annotations

import ctypes as C
from ctypes import byref, c_int, c_int64   # (by name: methods whose argument C is a number of clusters cannot reach the alias)
import errno
import os

import numpy as np

from . import _lib as L

ANNOT_REC = 12   # LDW_ANNOT_REC: int32 words of one k_annot_snp record


def fasta_check(code: int, path):
    """L.check for the FASTA feeder's entries: its two input errors become the ValueErrors ``snpdat.read_fasta`` raises, an unreadable
    path the OSError ``open`` would raise."""
    if code == L.LDW_OK:
        return
    msg = L.lib().ldw_last_error().decode("utf-8", "replace")
    if "does not contain any sequences" in msg:
        raise ValueError("File does not contain any sequences!")
    if "sequences are of different lengths" in msg:
        raise ValueError("Error! sequences are of different lengths!")
    if "cannot open" in msg:
        raise FileNotFoundError(errno.ENOENT, msg, str(path)) if not os.path.exists(path) else OSError(msg)
    raise L.LdwError(code, msg)


def _is_torch(x):
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda")


class Engine:
    def __init__(self, device: int = 0, stream=None):
        self._ctx = C.c_void_p()
        L.check(L.lib().ldw_ctx_create(int(device), C.byref(self._ctx)))
        self.device = int(device)
        self.L = self.N = 0
        if stream is not None:
            self.set_stream(stream)

    # -- lifetime ------------------------------------------------------------
    def close(self, trim: bool = False):
        """Destroy the context.  Its large device blocks go to the process-wide free list for the next engine (capped; trimmed to LDW_DEVPOOL_IDLE_GB when the
        process's last context goes); trim=True gives everything back to the runtime at once — for a process that shares the GPU with other allocators
        (torch, RCCL buffers, other ranks on the same device).

        Device views this engine handed out (``links_view``, ``sr_tail_extract(on_device=True)``) stay valid only until the context is
        destroyed, and destroying it waits for the engine's own streams only: synchronise every stream that reads them (a torch or RCCL
        stream) before calling close()."""
        if self._ctx:
            L.lib().ldw_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()
            if trim:
                n = C.c_int64(0)
                L.lib().ldw_host_trim(None, C.byref(n))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_stream(self, stream):
        """stream: a raw hipStream_t value (int), e.g. torch.cuda.current_stream().cuda_stream; None/0 = own stream.  Any kind of stream, between
        any two calls (ldw_ctx_set_stream waits for everything the context has queued); the stream is never destroyed by the engine."""
        L.check(L.lib().ldw_ctx_set_stream(self._ctx, C.c_void_p(int(stream) if stream else 0)))

    def sync(self):
        L.check(L.lib().ldw_ctx_sync(self._ctx))

    def last_timing(self):
        t = np.zeros(4)
        L.check(L.lib().ldw_ctx_last_timing(self._ctx, L.ptr(t)))
        return dict(gemm_ms=t[0], epilogue_ms=t[1], select_ms=t[2], total_ms=t[3])

    def gemm_stats(self, reset: bool = False):
        """Launches and EXECUTED int8 operations of the block-wide GEMMs since the last reset (ldw_gemm_stats)."""
        v = np.zeros(6)
        L.check(L.lib().ldw_gemm_stats(self._ctx, L.ptr(v), int(reset)))
        return dict(apx_launches=int(v[0]), apx_ops=float(v[1]), bits_launches=int(v[2]), bits_ops=float(v[3]), band_launches=int(v[4]),
                    apx_table_launches=int(v[5]))

    def hamming_stats(self):
        """What the last hamming_weights call did (ldw_hamming_stats): columns, stage times (HIP events), algorithmic bytes around the GEMM, host wall ms."""
        v = np.zeros(8)
        L.check(L.lib().ldw_hamming_stats(self._ctx, L.ptr(v)))
        return dict(columns=int(v[0]), k_padded=int(v[1]), pre_ms=float(v[2]), gemm_ms=float(v[3]), post_ms=float(v[4]), pre_bytes=float(v[5]), post_bytes=float(v[6]),
                    wall_ms=float(v[7]))

    def counters(self):
        v = np.zeros(8, dtype=np.int64)
        L.check(L.lib().ldw_ctx_counters2(self._ctx, L.ptr(v)))
        return dict(spec_misses=int(v[0]), fused_blocks=int(v[1]), unfused_blocks=int(v[2]), screen_violations=int(v[3]),
                    mixed_blocks=int(v[4]), apx_blocks=int(v[5]), apx_units_listed=int(v[6]), apx_pairs_listed=int(v[7]))

    def reset_speculation(self):
        """Forget the bucket guesses / threshold table earlier passes left behind: the next pass runs as a job's first pass."""
        L.check(L.lib().ldw_reset_speculation(self._ctx))

    def path_report(self):
        """Which execution path the blocks took so far and, if the approximate path is off, the gate that failed."""
        v = np.zeros(8, dtype=np.int64)
        buf = C.create_string_buffer(200)
        L.check(L.lib().ldw_path_report(self._ctx, L.ptr(v), buf, 200))
        return dict(apx_blocks=int(v[0]), mixed_blocks=int(v[1]), plain_blocks=int(v[2]), fused_blocks=int(v[3]), spec_misses=int(v[4]),
                    probe_blocks=int(v[5]), pairs_listed=int(v[6]), units_listed=int(v[7]), apx_gate=buf.value.decode())

    def form_report(self):
        """Kernel launches by form since the context was created (ldw_pair_form_report): the exact pair sums of the listed pairs (ldw_pairs.hip) walking set bits
        within 64 KB of LDS / with the 160-KB attribute, class-wise with LDS / global segment tables, and bit-row fills from global memory."""
        v = np.zeros(5, dtype=np.int64)
        L.check(L.lib().ldw_pair_form_report(self._ctx, L.ptr(v)))
        return dict(bits_lds64=int(v[0]), bits_lds160=int(v[1]), classwise_lds=int(v[2]), classwise_global=int(v[3]), fill_rows_global=int(v[4]))

    def pair_kernel_report(self):
        """Launches of the class-wise pair sums by kernel since the context was created (ldw_pair_kernel_report): a quarter-wave per pair
        (the default), a wave per pair (LDW_PAIR_WAVE=1, or segment tables in global memory)."""
        v = np.zeros(2, dtype=np.int64)
        L.check(L.lib().ldw_pair_kernel_report(self._ctx, L.ptr(v)))
        return dict(quarter_wave=int(v[0]), wave=int(v[1]))

    def set_prune(self, on: bool):
        """Tile pruning of the approximate path (default on): rows ordered by minor-state weight, rare x rare tiles never computed."""
        L.check(L.lib().ldw_set_prune(self._ctx, int(bool(on))))

    def prune_report(self):
        v = np.zeros(4, dtype=np.int64)
        L.check(L.lib().ldw_prune_report(self._ctx, L.ptr(v)))
        return dict(ordered_blocks=int(v[0]), tiles_pruned=int(v[1]), tiles_total=int(v[2]), on=bool(v[3]))

    def sr_pairs(self, blocks, sr_dist: float, n_rows: int | None = None):
        """(a, b) int32 CUDA tensors: the index columns of the short-range table of a pass over `blocks` (in their order), rebuilt from the
        positions alone (ldw_sr_pairs_fill).  What rank 0 of a multi-GPU run does instead of receiving them."""
        import torch
        bl = L.as_c(blocks, np.int32).reshape(-1, 4)
        n = C.c_int64(0)
        if n_rows is None:
            L.check(L.lib().ldw_sr_pairs_fill(self._ctx, L.ptr(bl), len(bl), float(sr_dist), None, None, 0, C.byref(n)))
            n_rows = int(n.value)
        dev = torch.device("cuda", self.device)
        a = torch.empty(max(1, n_rows), dtype=torch.int32, device=dev)
        b = torch.empty(max(1, n_rows), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        L.check(L.lib().ldw_sr_pairs_fill(self._ctx, L.ptr(bl), len(bl), float(sr_dist), C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), n_rows, C.byref(n)))
        assert int(n.value) == n_rows, (int(n.value), n_rows)
        return a[:n_rows], b[:n_rows]

    def set_span(self, on: bool, max_blocks: int = 0, corners: bool = False, diag_split: bool = False):
        """Spans (default on): consecutive long-range-only block pairs of one block row run as one launch sequence; results never depend on it.
        corners / diag_split: the corner-span and split-diagonal-block variants, measured slower and removed: LdwError (LDW_ERR_STATE)."""
        L.check(L.lib().ldw_set_span(self._ctx, (1 if on else 0) | (2 if (on and corners) else 0) | (4 if (on and diag_split) else 0), int(max_blocks)))

    def span_report(self):
        v = np.zeros(4, dtype=np.int64)
        L.check(L.lib().ldw_span_report(self._ctx, L.ptr(v)))
        return dict(spans=int(v[0]), blocks=int(v[1]), redone=int(v[2]), on=bool(v[3]))

    def overflow_report(self):
        """Blocks / span segments redone because a device list overflowed: pair lists, the maybe list (worst-case sized: 0 unless
        LDW_MAYBE_CAP is set), and whether the maybe list is switched off for the rest of the pass."""
        v = np.zeros(4, dtype=np.int64)
        L.check(L.lib().ldw_overflow_report(self._ctx, L.ptr(v)))
        return dict(pair_list=int(v[0]), maybe_list=int(v[1]), maybe_off=bool(v[2]), maybe_entries=int(v[3]))

    def slot_report(self):
        """The per-slot device buffers of a block's launch chain: reallocations since the context was created and the bytes held now."""
        v = np.zeros(6, dtype=np.int64)
        L.check(L.lib().ldw_slot_report(self._ctx, L.ptr(v)))
        return dict(grown=int(v[0]), units=int(v[1]), packs=int(v[2]), pairs=int(v[3]), bins=int(v[4]), mini=int(v[5]))

    @staticmethod
    def set_pair_cap(cap: int):
        """Tests only: a fixed capacity of the approximate path's pair lists (0: automatic), process-wide."""
        L.check(L.lib().ldw_set_pair_cap(int(cap)))

    def snp_bounds(self):
        """(L, 2, 2) array [snp, RXY reading (intended, reference), partner kind (2, 3 states)]: the largest MI the SNP can reach."""
        out = np.zeros(4 * self.L)
        L.check(L.lib().ldw_snp_bounds(self._ctx, L.ptr(out), out.size))
        return out.reshape(self.L, 2, 2)

    # -- test hooks: the bounds of the default path as functions (BOUNDS.md; csrc/ldw_debug.hip) --------------------
    APX_PARAM_NAMES = ("F", "e_last", "delta", "lost_units", "total_fixed", "neff", "apx_EG", "apx_dfac", "apx_s1", "apx_c1", "apx_W", "apx_unit", "scr_scale",
                       "scr_shift_exact", "scr_scale_exact", "flags", "lo_abs_sum", "lo_bound", "apx_MU", "nlimbs")

    def debug_apx_params(self, want_weights: bool = True):
        """(params[20], V[N], V'[N]): the constants of the approximate screen's bound for the current weights (names: APX_PARAM_NAMES) and, per sequence, the
        exact fixed-point weight and its dual-digit approximation."""
        out = np.zeros(20)
        V = np.zeros(self.N if want_weights else 0, dtype=np.int64)
        Va = np.zeros(self.N if want_weights else 0, dtype=np.int64)
        L.check(L.lib().ldw_debug_apx_params(self._ctx, L.ptr(out), L.ptr(V) if want_weights else None, L.ptr(Va) if want_weights else None, self.N))
        return out, V, Va

    def debug_rows(self):
        """(row0[L + 1], slot_meta[L]): first indicator row of every SNP; rows | uqe flags << 3 | slot states << 8."""
        row0 = np.zeros(self.L + 1, dtype=np.int32)
        meta = np.zeros(self.L, dtype=np.uint32)
        L.check(L.lib().ldw_debug_rows(self._ctx, L.ptr(row0), L.ptr(meta), self.L + 1))
        return row0, meta

    def debug_apx_gemm(self, rows_t, rows_f, grid_wgs: int | None = None):
        """gemm_apx_kernel over the given indicator rows: int32 [len(rows_t), len(rows_f)] sums of the dual-digit weights in units of 2^e_last.
        grid_wgs: through the kernel's list launch with that many workgroups (ldw_debug_apx_gemm_list) instead of the 2-D launch."""
        rt = np.ascontiguousarray(rows_t, dtype=np.int32)
        rf = np.ascontiguousarray(rows_f, dtype=np.int32)
        out = np.zeros((len(rt), len(rf)), dtype=np.int32)
        if grid_wgs is None:
            L.check(L.lib().ldw_debug_apx_gemm(self._ctx, L.ptr(rt), len(rt), L.ptr(rf), len(rf), L.ptr(out)))
        else:
            L.check(L.lib().ldw_debug_apx_gemm_list(self._ctx, L.ptr(rt), len(rt), L.ptr(rf), len(rf), int(grid_wgs), L.ptr(out)))
        return out

    APX_FUSED_FILL = 0xA5                                                             # LDW_DEBUG_APX_FUSED_FILL: every byte no kernel wrote
    APX_FUSED_FILL32 = int(np.frombuffer(bytes([0xA5] * 4), dtype=np.int32)[0])
    APX_MAYBE_MAX = 96                                                                # LDW_DEBUG_APX_MAYBE_MAX (the library's build asserts it)

    def debug_apx_gemm_fused(self, rows_t, rows_f, bin_t, bin_f, tab, rflag_t=None, rflag_f=None, sr_mask=None, lower_only: bool = False, prune: bool = False,
                             grid_wgs: int = 0, maybe_cap: int = -1, out=None):
        """The fused launches of the approximate GEMM on caller-made inputs (ldw_debug_apx_gemm_fused): the table test of the epilogue and, with prune, the
        live-tile pass in front of the list launch (grid_wgs workgroups, 0: the default path's grid).  bin_t / bin_f: a table bin 0..63 or 255 per row;
        rflag_t / rflag_f: pruning flags per row (both or neither); tab: int32 [64, 64, 2] (Lq, Hq); sr_mask: uint8 [RTpad / 128, RFpad / 64]; maybe_cap: -1 =
        no maybe list.  Returns a dict of the raw buffers — G int32 [RTpad, RFpad], clean uint8 [RTpad / 32, RFpad / 64], tiles uint32 [tiles], maybe int32
        [max(maybe_cap, 0), 3] — whatever no kernel wrote holds APX_FUSED_FILL bytes, and n_live, pruned, maybe_n, beyond_cap (bytes written behind the maybe list's capacity: 0).  out: a dict of such arrays to write
        into (a refused call leaves them untouched)."""
        rt = np.ascontiguousarray(rows_t, dtype=np.int32)
        rf = np.ascontiguousarray(rows_f, dtype=np.int32)
        bt = np.ascontiguousarray(bin_t, dtype=np.uint8)
        bf = np.ascontiguousarray(bin_f, dtype=np.uint8)
        assert bt.shape == rt.shape and bf.shape == rf.shape
        ft = None if rflag_t is None else np.ascontiguousarray(rflag_t, dtype=np.uint8)
        ff = None if rflag_f is None else np.ascontiguousarray(rflag_f, dtype=np.uint8)
        assert (ft is None or ft.shape == rt.shape) and (ff is None or ff.shape == rf.shape)
        tb = np.ascontiguousarray(tab, dtype=np.int32)
        assert tb.shape == (64, 64, 2), tb.shape
        RTpad, RFpad = -(-len(rt) // 128) * 128, -(-len(rf) // 128) * 128
        mask = None if sr_mask is None else np.ascontiguousarray(sr_mask, dtype=np.uint8)
        assert mask is None or mask.shape == (RTpad // 128, RFpad // 64), mask.shape
        if out is None:
            out = dict(G=np.zeros((RTpad, RFpad), dtype=np.int32), clean=np.zeros((RTpad // 32, RFpad // 64), dtype=np.uint8),
                       tiles=np.zeros((RTpad // 128) * (RFpad // 64), dtype=np.uint32), maybe=np.zeros((max(int(maybe_cap), 0), 3), dtype=np.int32))
        counts = np.zeros(4, dtype=np.int64)
        L.check(L.lib().ldw_debug_apx_gemm_fused(self._ctx, L.ptr(rt), len(rt), L.ptr(rf), len(rf), L.ptr(bt), L.ptr(bf), L.ptr(ft), L.ptr(ff), L.ptr(tb), L.ptr(mask),
                                                 int(bool(lower_only)), int(bool(prune)), int(grid_wgs), int(maybe_cap), L.ptr(out["G"]), L.ptr(out["clean"]),
                                                 L.ptr(out["tiles"]), L.ptr(out["maybe"]) if out["maybe"].size else None, L.ptr(counts)))
        return dict(out, n_live=int(counts[0]), pruned=int(counts[1]), maybe_n=int(counts[2]), beyond_cap=int(counts[3]))

    LIMB_GEMM_FILL = int(np.frombuffer(bytes([0xA5] * 8), dtype=np.int64)[0])
    LO_UNITS_FILL = int(np.frombuffer(bytes([0xA5] * 4), dtype=np.int32)[0])

    def debug_limb_gemm(self, rows_t, rows_f, engine: int = 0, limb0: int = 0, nlimbs: int | None = None, lower_only: bool = False, by0: int = 0, by1: int = -1,
                        tile_mask=None, tile_list=None, out=None):
        """The exact co-occurrence GEMMs over the given indicator rows (ldw_debug_limb_gemm): engine 0 = gemm_bits_kernel with the weight limbs limb0 ..
        limb0 + nlimbs - 1 (None: all from limb0 up), engine 1 = k_cooc_popc.  lower_only, the strip by0..by1 of tile rows, tile_mask [RTpad / 128, RFpad / 64]
        and tile_list (by << 16 | bx; an empty list launches nothing) are handed to the launch as they are.  Returns int64 [len(rows_t), len(rows_f)]; whatever
        no kernel wrote holds LIMB_GEMM_FILL.  out: an array to write into (a refused call leaves it untouched)."""
        rt = np.ascontiguousarray(rows_t, dtype=np.int32)
        rf = np.ascontiguousarray(rows_f, dtype=np.int32)
        if nlimbs is None:
            nlimbs = int(self.debug_apx_params(want_weights=False)[0][19]) - int(limb0)
        if out is None:
            out = np.zeros((len(rt), len(rf)), dtype=np.int64)
        assert out.dtype == np.int64 and out.shape == (len(rt), len(rf)) and out.flags.c_contiguous
        mask = None if tile_mask is None else np.ascontiguousarray(tile_mask, dtype=np.uint8)
        if mask is not None:
            assert mask.shape == (-(-len(rt) // 128), 2 * -(-len(rf) // 128)), mask.shape
        tl = None if tile_list is None else np.ascontiguousarray(tile_list, dtype=np.uint32).reshape(-1)
        n_tl = 0 if tl is None else len(tl)
        if tl is not None and n_tl == 0:
            tl = np.zeros(1, dtype=np.uint32)      # (a non-null list of no entries)
        L.check(L.lib().ldw_debug_limb_gemm(self._ctx, int(engine), L.ptr(rt), len(rt), L.ptr(rf), len(rf), int(limb0), int(nlimbs), int(bool(lower_only)), int(by0), int(by1),
                                            L.ptr(mask), L.ptr(tl), n_tl, L.ptr(out)))
        return out

    def debug_lo_units(self, from_snps, to_snps, lists, launch: bool = True):
        """The gathered low-limb GEMM on caller-made unit lists (ldw_debug_lo_units).  from_snps[64 * ntiles]: the SNPs of the from-tiles' lanes (-1: a padding
        lane); to_snps[nt]: the SNP of every column slot; lists[tile][lc]: the listed column slots of row-slot class lc (0, 1, 2).  Returns a dict: glo (the raw
        int32 buffer, None with launch = False; what the kernel did not write holds LO_UNITS_FILL), tile_base, cmax, rowbase, uoff, RTlo, n_tf."""
        fs = np.ascontiguousarray(from_snps, dtype=np.int32).reshape(-1)
        ts = np.ascontiguousarray(to_snps, dtype=np.int32).reshape(-1)
        assert len(fs) % 64 == 0 and len(fs) > 0
        ntiles = len(fs) // 64
        assert len(lists) == ntiles and all(len(x) == 3 for x in lists)
        counts = np.array([[len(x[lc]) for lc in range(3)] for x in lists], dtype=np.uint32)
        flat = [np.asarray(x[lc], dtype=np.int32).reshape(-1) for x in lists for lc in range(3)]
        slots = np.ascontiguousarray(np.concatenate(flat + [np.zeros(1, dtype=np.int32)]))
        geom = np.zeros(8, dtype=np.int32)
        cmax = np.zeros(ntiles, dtype=np.int32)
        tbase = np.zeros(ntiles, dtype=np.int64)
        total = C.c_int64(0)

        def call(glo, cap):
            L.check(L.lib().ldw_debug_lo_units(self._ctx, L.ptr(fs), ntiles, L.ptr(ts), len(ts), L.ptr(counts), L.ptr(slots), L.ptr(geom), L.ptr(cmax), L.ptr(tbase),
                                               C.byref(total), L.ptr(glo), cap))

        call(None, 0)
        glo = None
        if launch:
            glo = np.zeros(int(total.value), dtype=np.int32)
            call(glo, len(glo))
        return dict(glo=glo, tile_base=tbase, cmax=cmax, rowbase=geom[0:3].copy(), uoff=geom[3:6].copy(), RTlo=int(geom[6]), n_tf=int(geom[7]), glo_total=int(total.value))

    PAIR_PATHS, PAIR_SHARDS = 5, 8
    PAIR_FORMS = ("auto", "quarter_wave", "wave_lds", "wave_global", "bits")
    PAIR_SUMS_FILL = int(np.frombuffer(bytes([0xA5] * 8), dtype=np.int64)[0])

    def debug_pair_sums(self, counts, snp_a, snp_b, form: int = 0, grid_wgs: int = 0):
        """The exact joint sums of caller-made pair lists by the sum kernels of ldw_pairs.hip alone (ldw_debug_pair_sums): counts[40] entries per list (list = path * 8 +
        shard; a count above the capacity is clamped by the kernels), snp_a / snp_b [40, cap] the SNPs of the entries.  form: an index of PAIR_FORMS
        (0: what the default path would launch), grid_wgs: gridDim.x of both launches (0: the default path's).  Returns (sums int64 [40, cap, 16], the
        form that ran); whatever the kernels did not write holds PAIR_SUMS_FILL."""
        nl = self.PAIR_PATHS * self.PAIR_SHARDS
        cnt = np.ascontiguousarray(counts, dtype=np.uint32).reshape(nl)
        a = np.ascontiguousarray(snp_a, dtype=np.int32)
        b = np.ascontiguousarray(snp_b, dtype=np.int32)
        assert a.shape == b.shape and a.size % nl == 0, (a.shape, b.shape)
        cap = a.size // nl
        out = np.zeros((nl, cap, 16), dtype=np.int64)
        ran = C.c_int(0)
        L.check(L.lib().ldw_debug_pair_sums(self._ctx, int(form), int(grid_wgs), cap, L.ptr(cnt), L.ptr(a), L.ptr(b), L.ptr(out), C.byref(ran)))
        return out, int(ran.value)

    # -- LD decay ---------------------------------------------------
    @staticmethod
    def _decay_cuts(cuts):
        cu = np.zeros(0) if cuts is None else L.as_c(cuts, np.float64).ravel()
        return cu, min(len(cu), 1 << 20)

    def mi_profile(self, blocks, cuts, mi_shift: int = 3, quirk=L.QUIRK_REFERENCE):
        """The histogram, circular distance bin x MI bucket, of EVERY SNP pair of ``blocks`` ((nb, 4) rows as make_blocks emits them), with the largest MI of
        every distance bin (ldw_mi_profile).  ``cuts``: ascending distances; bin k holds the pairs with cuts[k-1] < len <= cuts[k].  Returns a dict: ``hist``
        uint64 (len(cuts) + 1, 4096 >> mi_shift), ``max`` float64 (NaN for an empty bin), ``n_pairs``.  The link tables stay as they are."""
        bl = L.as_c(blocks, np.int32).reshape(-1, 4)
        cu, n_cut = self._decay_cuts(cuts)
        nb = 4096 >> mi_shift if 0 <= int(mi_shift) <= 6 else 1
        hist = np.zeros((min(n_cut, 1023) + 1, nb), dtype=np.uint64)
        mx = np.full(hist.shape[0], np.nan)
        n = C.c_int64(0)
        L.check(L.lib().ldw_mi_profile(self._ctx, L.ptr(bl), len(bl), int(quirk), L.ptr(cu) if n_cut else None, n_cut, int(mi_shift), L.ptr(hist), L.ptr(mx),
                                       C.byref(n)))
        return dict(hist=hist, max=mx, n_pairs=int(n.value))

    def decay_report(self):
        """Of the last mi_profile (ldw_decay_report): patches of the histogram kernel, those that took route B, pairs outside their patch's bound, blocks."""
        v = np.zeros(4, dtype=np.int64)
        L.check(L.lib().ldw_decay_report(self._ctx, L.ptr(v)))
        return dict(patches=int(v[0]), route_b=int(v[1]), outside=int(v[2]), blocks=int(v[3]))

    def debug_profile_hist(self, mi, pos_f, pos_t, g, diag, cuts, mi_shift: int = 3, route: int = 0):
        """The histogram kernel of mi_profile on caller-made values (ldw_debug_profile_hist): ``mi`` (nf, nt) (stored column-major for the call), the positions
        of the two sides, the genome length, ``diag`` (pairs a > b of a square block) or not (pairs a != b).  route 0: every patch chooses, 1: the LDS window
        (LdwError LDW_ERR_ARG where it does not fit), 2: wave-aggregated global adds.  Returns the dict of mi_profile plus ``stats`` (patches, route-B patches,
        pairs outside their patch's bound)."""
        m = np.asarray(mi, dtype=np.float64)
        assert m.ndim == 2, m.shape
        nf, nt = m.shape
        mf = np.asfortranarray(m)
        pf, pt = L.as_c(pos_f, np.int32).ravel(), L.as_c(pos_t, np.int32).ravel()
        assert len(pf) == nf and len(pt) == nt, (len(pf), len(pt), m.shape)
        cu, n_cut = self._decay_cuts(cuts)
        nb = 4096 >> mi_shift if 0 <= int(mi_shift) <= 6 else 1
        hist = np.zeros((min(n_cut, 1023) + 1, nb), dtype=np.uint64)
        mx = np.full(hist.shape[0], np.nan)
        n, st = C.c_int64(0), np.zeros(3, dtype=np.int64)
        L.check(L.lib().ldw_debug_profile_hist(self._ctx, L.ptr(mf), nf, nt, L.ptr(pf), L.ptr(pt), float(g), int(bool(diag)), L.ptr(cu) if n_cut else None, n_cut,
                                               int(mi_shift), int(route), L.ptr(hist), L.ptr(mx), C.byref(n), L.ptr(st)))
        return dict(hist=hist, max=mx, n_pairs=int(n.value), stats=st)

    # -- per-SNP MI summary -----------------------------------------
    def mi_snp_summary(self, blocks, sr_dist, thr=(np.inf, np.inf), quirk=L.QUIRK_REFERENCE):
        """Per SNP and distance class (0: len <= sr_dist, 1: beyond) over EVERY SNP pair of ``blocks`` (ldw_mi_snp_summary), each pair adding to both of its
        SNPs: ``n`` the partners, ``sumq`` the sum of llrint(mi 2^40), ``max`` the largest MI (NaN where n == 0), ``nge`` the partners with mi >= thr[class] —
        each (2, L) — and ``npairs`` (2,) the pairs of each class.  The link tables stay as they are."""
        bl = L.as_c(blocks, np.int32).reshape(-1, 4)
        th = L.as_c(thr, np.float64).reshape(2)
        n, sumq, nge = (np.zeros((2, self.L), dtype=np.int64) for _ in range(3))
        mx = np.full((2, self.L), np.nan)
        npairs = np.zeros(2, dtype=np.int64)
        L.check(L.lib().ldw_mi_snp_summary(self._ctx, L.ptr(bl), len(bl), int(quirk), float(sr_dist), L.ptr(th), L.ptr(n), L.ptr(sumq), L.ptr(mx), L.ptr(nge),
                                           L.ptr(npairs)))
        return dict(n=n, sumq=sumq, max=mx, nge=nge, npairs=npairs)

    def snp_summary_report(self):
        """Of the last mi_snp_summary (ldw_snp_summary_report): patches the summary kernel visited, those on the general route, pairs off their patch's class,
        values the fixed point refused, blocks."""
        v = np.zeros(5, dtype=np.int64)
        L.check(L.lib().ldw_snp_summary_report(self._ctx, L.ptr(v)))
        return dict(patches=int(v[0]), general=int(v[1]), off_class=int(v[2]), refused=int(v[3]), blocks=int(v[4]))

    def debug_snp_summary(self, mi, pos_f, pos_t, g, diag, sr_dist, thr=(np.inf, np.inf), route: int = 0):
        """The kernel of mi_snp_summary on caller-made values (ldw_debug_snp_summary): ``mi`` (nf, nt) (stored column-major for the call), the positions of
        the two sides, the genome length, ``diag`` (pairs a > b of a square block) or not (pairs a != b).  route 0: every patch chooses, 1: single class
        (LdwError LDW_ERR_ARG where the bound does not say), 2: both classes carried.  Returns ``rows`` and ``cols``, each a dict of n, sumq, max, nge with
        shapes (2, nf) and (2, nt) — what the pairs add to their from-SNPs and to their to-SNPs —, ``npairs`` (2,) and ``stats`` (patches visited, general-route
        patches, pairs off their patch's class, values refused)."""
        m = np.asarray(mi, dtype=np.float64)
        assert m.ndim == 2, m.shape
        nf, nt = m.shape
        mf = np.asfortranarray(m)
        pf, pt = L.as_c(pos_f, np.int32).ravel(), L.as_c(pos_t, np.int32).ravel()
        assert len(pf) == nf and len(pt) == nt, (len(pf), len(pt), m.shape)
        th = L.as_c(thr, np.float64).reshape(2)
        side = lambda k: dict(n=np.zeros((2, k), dtype=np.int64), sumq=np.zeros((2, k), dtype=np.int64), max=np.full((2, k), np.nan),
                              nge=np.zeros((2, k), dtype=np.int64))
        rows, cols = side(nf), side(nt)
        npairs, st = np.zeros(2, dtype=np.int64), np.zeros(4, dtype=np.int64)
        L.check(L.lib().ldw_debug_snp_summary(self._ctx, L.ptr(mf), nf, nt, L.ptr(pf), L.ptr(pt), float(g), int(bool(diag)), float(sr_dist), L.ptr(th), int(route),
                                              *[L.ptr(s[k]) for s in (rows, cols) for k in ("n", "sumq", "max", "nge")], L.ptr(npairs), L.ptr(st)))
        return dict(rows=rows, cols=cols, npairs=npairs, stats=st)

    # -- selection by a corrected score -----------------------------
    def mi_score_scan(self, blocks, sr_dist, cls_mask, w, quirk=L.QUIRK_REFERENCE):
        """Over EVERY SNP pair of ``blocks`` inside the class mask (1: len <= sr_dist, 2: beyond, 3: both), with the score s = mi - w[a] w[b]
        (ldw_mi_score_scan): ``hist`` uint64 (4096,) the pairs per ``mi_bucket(s)``, ``best`` float64 (L,) the largest score of every SNP over its partners (NaN
        where none) and ``npairs`` the pairs inside the mask.  ``w`` (L,) must be finite.  The link tables stay as they are."""
        bl = L.as_c(blocks, np.int32).reshape(-1, 4)
        wv = L.as_c(w, np.float64).reshape(self.L)
        hist, best, n = np.zeros(4096, dtype=np.uint64), np.full(self.L, np.nan), C.c_int64(0)
        L.check(L.lib().ldw_mi_score_scan(self._ctx, L.ptr(bl), len(bl), int(quirk), float(sr_dist), int(cls_mask), L.ptr(wv), L.ptr(hist), L.ptr(best), C.byref(n)))
        return dict(hist=hist, best=best, npairs=int(n.value))

    @staticmethod
    def _link_lists(cap):
        cap = int(cap)
        return (np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32), np.zeros(cap), np.zeros(cap)) if cap > 0 else (None, None, None, None)

    def mi_score_links(self, blocks, sr_dist, cls_mask, w, thr, cap: int = 0, best_in=None, quirk=L.QUIRK_REFERENCE):
        """The pairs of ``mi_score_scan``'s pair set with s >= ``thr`` (ldw_mi_score_links): ``a`` / ``b`` the from-SNP and the to-SNP (global, 0-based), ``mi``,
        ``score``, in no stated order, and ``count``, exact whatever ``cap`` is.  ``cap`` = 0 only counts; a count above ``cap`` raises LdwError LDW_ERR_SIZE,
        which carries the count as ``.count``.  With ``best_in`` (L,) — the ``best`` of a scan with the same arguments — ``partner`` int32 (L,) is the smallest
        partner of every SNP whose score has the bits of best_in, -1 where there is none."""
        bl = L.as_c(blocks, np.int32).reshape(-1, 4)
        wv = L.as_c(w, np.float64).reshape(self.L)
        a, b, mi, sc = self._link_lists(cap)
        bi = None if best_in is None else L.as_c(best_in, np.float64).reshape(self.L)
        partner = None if bi is None else np.full(self.L, -1, dtype=np.int32)
        n = C.c_int64(0)
        try:
            L.check(L.lib().ldw_mi_score_links(self._ctx, L.ptr(bl), len(bl), int(quirk), float(sr_dist), int(cls_mask), L.ptr(wv), float(thr), L.ptr(bi), max(int(cap), 0),
                                               L.ptr(a), L.ptr(b), L.ptr(mi), L.ptr(sc), C.byref(n), L.ptr(partner)))
        except L.LdwError as e:
            e.count = int(n.value)
            raise
        k = int(n.value)
        cut = (lambda x: None if x is None else x[:k])
        return dict(a=cut(a), b=cut(b), mi=cut(mi), score=cut(sc), count=k, partner=partner)

    def score_select_report(self):
        """Of the last mi_score_scan or mi_score_links (ldw_score_select_report): patches the kernel visited, NaN scores, blocks."""
        v = np.zeros(3, dtype=np.int64)
        L.check(L.lib().ldw_score_select_report(self._ctx, L.ptr(v)))
        return dict(patches=int(v[0]), nan_scores=int(v[1]), blocks=int(v[2]))

    @staticmethod
    def _debug_block(mi, pos_f, pos_t, w_f, w_t):
        m = np.asarray(mi, dtype=np.float64)
        assert m.ndim == 2, m.shape
        nf, nt = m.shape
        pf, pt = L.as_c(pos_f, np.int32).ravel(), L.as_c(pos_t, np.int32).ravel()
        wf, wt = L.as_c(w_f, np.float64).ravel(), L.as_c(w_t, np.float64).ravel()
        assert len(pf) == nf == len(wf) and len(pt) == nt == len(wt), (len(pf), len(pt), len(wf), len(wt), m.shape)
        return np.asfortranarray(m), nf, nt, pf, pt, wf, wt

    def debug_score_scan(self, mi, pos_f, pos_t, g, diag, sr_dist, cls_mask, w_f, w_t):
        """The kernel of mi_score_scan on caller-made values (ldw_debug_score_scan): ``mi`` (nf, nt) (stored column-major for the call), the positions and the
        weights of the two sides, the genome length, ``diag`` (pairs a > b of a square block) or not (pairs a != b).  Returns ``hist``, ``best_f`` (nf,) and
        ``best_t`` (nt,) — the two sides apart —, ``npairs`` and ``stats`` (patches visited, NaN scores)."""
        mf, nf, nt, pf, pt, wf, wt = self._debug_block(mi, pos_f, pos_t, w_f, w_t)
        hist, bf, bt = np.zeros(4096, dtype=np.uint64), np.full(nf, np.nan), np.full(nt, np.nan)
        n, st = C.c_int64(0), np.zeros(2, dtype=np.int64)
        L.check(L.lib().ldw_debug_score_scan(self._ctx, L.ptr(mf), nf, nt, L.ptr(pf), L.ptr(pt), float(g), int(bool(diag)), float(sr_dist), int(cls_mask), L.ptr(wf),
                                             L.ptr(wt), L.ptr(hist), L.ptr(bf), L.ptr(bt), C.byref(n), L.ptr(st)))
        return dict(hist=hist, best_f=bf, best_t=bt, npairs=int(n.value), stats=st)

    def debug_score_links(self, mi, pos_f, pos_t, g, diag, sr_dist, cls_mask, id_f, id_t, w_f, w_t, thr, cap: int = 0, best_f=None, best_t=None):
        """The kernel of mi_score_links on caller-made values (ldw_debug_score_links), as debug_score_scan; ``id_f`` / ``id_t`` the global ids of the two sides.
        Returns the dict of mi_score_links with ``partner_f`` (nf,) and ``partner_t`` (nt,) in place of ``partner`` (None without ``best_f`` / ``best_t``) and
        ``stats`` (patches visited, NaN scores)."""
        mf, nf, nt, pf, pt, wf, wt = self._debug_block(mi, pos_f, pos_t, w_f, w_t)
        idf, idt = L.as_c(id_f, np.int32).ravel(), L.as_c(id_t, np.int32).ravel()
        assert len(idf) == nf and len(idt) == nt and (best_f is None) == (best_t is None), (len(idf), len(idt))
        a, b, mo, sc = self._link_lists(cap)
        bf = None if best_f is None else L.as_c(best_f, np.float64).reshape(nf)
        bt = None if best_t is None else L.as_c(best_t, np.float64).reshape(nt)
        prf = None if bf is None else np.full(nf, -1, dtype=np.int32)
        prt = None if bt is None else np.full(nt, -1, dtype=np.int32)
        n, st = C.c_int64(0), np.zeros(2, dtype=np.int64)
        try:
            L.check(L.lib().ldw_debug_score_links(self._ctx, L.ptr(mf), nf, nt, L.ptr(pf), L.ptr(pt), float(g), int(bool(diag)), float(sr_dist), int(cls_mask), L.ptr(idf),
                                                  L.ptr(idt), L.ptr(wf), L.ptr(wt), float(thr), L.ptr(bf), L.ptr(bt), max(int(cap), 0), L.ptr(a), L.ptr(b), L.ptr(mo),
                                                  L.ptr(sc), C.byref(n), L.ptr(prf), L.ptr(prt), L.ptr(st)))
        except L.LdwError as e:
            e.count = int(n.value)
            raise
        k = int(n.value)
        cut = (lambda x: None if x is None else x[:k])
        return dict(a=cut(a), b=cut(b), mi=cut(mo), score=cut(sc), count=k, partner_f=prf, partner_t=prt, stats=st)

    # -- the segment map --------------------------------------------
    @staticmethod
    def _segmap_side(S):
        return int(S) if 1 <= int(S) <= 8192 else 1      # (an S the library refuses: any shape will do)

    @staticmethod
    def _segmap_outputs(S):
        S = Engine._segmap_side(S)
        n, nge, lo, hi = (np.zeros((S, S), dtype=np.int64) for _ in range(4))
        return n, nge, lo, hi, np.full((S, S), np.nan)

    def _segmap_vectors(self, seg, w):
        sg = L.as_c(seg, np.int32).ravel()
        wv = None if w is None else L.as_c(w, np.float64).ravel()
        if self.L and (len(sg) != self.L or (wv is not None and len(wv) != self.L)):      # (without an alignment the library refuses the call itself)
            raise ValueError(f"seg and w take one entry per SNP ({self.L}), got {len(sg)}" + ("" if wv is None else f" and {len(wv)}"))
        return sg, wv

    def mi_segment_map(self, blocks, seg, S, sr_dist, cls_mask, w=None, thr=np.inf, quirk=L.QUIRK_REFERENCE):
        """Over EVERY SNP pair of ``blocks`` inside the class mask (1: len <= sr_dist, 2: beyond, 3: both), per cell (min(seg[a], seg[b]), max(seg[a], seg[b]))
        of the value v = mi, or mi - w[a] w[b] with ``w`` (ldw_mi_segment_map): ``n`` the pairs, ``nge`` the pairs with v >= thr, ``sum_lo`` / ``sum_hi`` the
        two words of the sum of llrint(v 2^40) (the exact sum is sum_hi 2^24 + sum_lo), each int64 (S, S), ``max`` float64 (S, S) the largest value (NaN where
        n == 0) and ``npairs``.  ``seg`` (L,) in -1..S-1; a pair with a SNP at -1 takes no part.  Only cells with row <= column are written.  The link tables
        stay as they are."""
        bl = L.as_c(blocks, np.int32).reshape(-1, 4)
        sg, wv = self._segmap_vectors(seg, w)
        n, nge, lo, hi, mx = self._segmap_outputs(S)
        npairs = C.c_int64(0)
        L.check(L.lib().ldw_mi_segment_map(self._ctx, L.ptr(bl), len(bl), int(quirk), L.ptr(sg), int(S), float(sr_dist), int(cls_mask), L.ptr(wv), float(thr), L.ptr(n),
                                           L.ptr(nge), L.ptr(lo), L.ptr(hi), L.ptr(mx), C.byref(npairs)))
        return dict(n=n, nge=nge, sum_lo=lo, sum_hi=hi, max=mx, npairs=int(npairs.value))

    def mi_segment_best(self, blocks, seg, S, sr_dist, cls_mask, max_in, w=None, quirk=L.QUIRK_REFERENCE):
        """Per cell of ``mi_segment_map``'s pair set the smallest packed pair (min(a, b) << 32 | max(a, b), uint64 (S, S)) whose value has the bits of
        ``max_in`` (S, S) (ldw_mi_segment_best); all-ones where max_in is NaN or nothing matches.  With ``max_in`` the ``max`` of a map call with the same
        arguments it names the pair behind each maximum."""
        bl = L.as_c(blocks, np.int32).reshape(-1, 4)
        sg, wv = self._segmap_vectors(seg, w)
        S_ = self._segmap_side(S)
        mi_ = L.as_c(max_in, np.float64).reshape(S_, S_)
        pair = np.full((S_, S_), np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
        L.check(L.lib().ldw_mi_segment_best(self._ctx, L.ptr(bl), len(bl), int(quirk), L.ptr(sg), int(S), float(sr_dist), int(cls_mask), L.ptr(wv), L.ptr(mi_), L.ptr(pair)))
        return pair

    def segment_map_report(self):
        """Of the last mi_segment_map or mi_segment_best (ldw_segment_map_report): patches the kernel visited, those on route 2, values the fixed point
        refused, NaN values, blocks."""
        v = np.zeros(5, dtype=np.int64)
        L.check(L.lib().ldw_segment_map_report(self._ctx, L.ptr(v)))
        return dict(patches=int(v[0]), general=int(v[1]), refused=int(v[2]), nan_values=int(v[3]), blocks=int(v[4]))

    @staticmethod
    def _segmap_block(mi, pos_f, pos_t, seg_f, seg_t, w_f, w_t):
        m = np.asarray(mi, dtype=np.float64)
        assert m.ndim == 2, m.shape
        nf, nt = m.shape
        pf, pt = L.as_c(pos_f, np.int32).ravel(), L.as_c(pos_t, np.int32).ravel()
        sf, st = L.as_c(seg_f, np.int32).ravel(), L.as_c(seg_t, np.int32).ravel()
        wf = None if w_f is None else L.as_c(w_f, np.float64).ravel()
        wt = None if w_t is None else L.as_c(w_t, np.float64).ravel()
        assert len(pf) == nf == len(sf) and len(pt) == nt == len(st), (len(pf), len(pt), len(sf), len(st), m.shape)
        assert (wf is None or len(wf) == nf) and (wt is None or len(wt) == nt)
        return np.asfortranarray(m), nf, nt, pf, pt, sf, st, wf, wt

    def debug_segment_map(self, mi, pos_f, pos_t, g, diag, seg_f, seg_t, S, sr_dist, cls_mask, w_f=None, w_t=None, thr=np.inf, route: int = 0):
        """The kernel of mi_segment_map on caller-made values (ldw_debug_segment_map): ``mi`` (nf, nt) (stored column-major for the call), the positions and
        the segments of the two sides, the genome length, ``diag`` (pairs a > b of a square block) or not (pairs a != b); the weights of the two sides both or
        neither.  route 0: every patch chooses, 1: the LDS window of runs (LdwError LDW_ERR_ARG where a patch does not fit), 2: per-pair global operations.
        Returns the dict of mi_segment_map plus ``stats`` (patches visited, route-2 patches, values refused, NaN values)."""
        mf, nf, nt, pf, pt, sf, st, wf, wt = self._segmap_block(mi, pos_f, pos_t, seg_f, seg_t, w_f, w_t)
        n, nge, lo, hi, mx = self._segmap_outputs(S)
        npairs, stats = C.c_int64(0), np.zeros(4, dtype=np.int64)
        L.check(L.lib().ldw_debug_segment_map(self._ctx, L.ptr(mf), nf, nt, L.ptr(pf), L.ptr(pt), float(g), int(bool(diag)), L.ptr(sf), L.ptr(st), int(S), float(sr_dist),
                                              int(cls_mask), L.ptr(wf), L.ptr(wt), float(thr), int(route), L.ptr(n), L.ptr(nge), L.ptr(lo), L.ptr(hi), L.ptr(mx),
                                              C.byref(npairs), L.ptr(stats)))
        return dict(n=n, nge=nge, sum_lo=lo, sum_hi=hi, max=mx, npairs=int(npairs.value), stats=stats)

    def debug_segment_best(self, mi, pos_f, pos_t, g, diag, seg_f, seg_t, S, sr_dist, cls_mask, id_f, id_t, max_in, w_f=None, w_t=None, route: int = 0):
        """The kernel of mi_segment_best on caller-made values (ldw_debug_segment_best), as debug_segment_map; ``id_f`` / ``id_t`` the global ids of the two
        sides.  Returns ``pair`` uint64 (S, S) and ``stats``."""
        mf, nf, nt, pf, pt, sf, st, wf, wt = self._segmap_block(mi, pos_f, pos_t, seg_f, seg_t, w_f, w_t)
        idf, idt = L.as_c(id_f, np.int32).ravel(), L.as_c(id_t, np.int32).ravel()
        assert len(idf) == nf and len(idt) == nt, (len(idf), len(idt))
        S_ = self._segmap_side(S)
        mi_ = L.as_c(max_in, np.float64).reshape(S_, S_)
        pair = np.full((S_, S_), np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
        stats = np.zeros(4, dtype=np.int64)
        L.check(L.lib().ldw_debug_segment_best(self._ctx, L.ptr(mf), nf, nt, L.ptr(pf), L.ptr(pt), float(g), int(bool(diag)), L.ptr(sf), L.ptr(st), int(S), float(sr_dist),
                                               int(cls_mask), L.ptr(idf), L.ptr(idt), L.ptr(wf), L.ptr(wt), L.ptr(mi_), int(route), L.ptr(pair), L.ptr(stats)))
        return dict(pair=pair, stats=stats)

    def debug_screen_bound(self, kind: int, na: int, nb: int, g, pa, pb, pX, pY, rr, params, masks=None):
        """The engine's screen / evaluation device functions on caller-made joint tables (ldw_debug_screen_bound): kind 0 / 1 the approximate path's upper
        bounds (straight-line / predicated), 2 / 3 the fp32 MI of the exact-limb screens, 4 the fp64 value the engine emits."""
        g = np.ascontiguousarray(g, dtype=np.int64).reshape(-1, 16)
        n = len(g)
        pa = np.ascontiguousarray(pa, dtype=np.int64).reshape(n, 5)
        pb = np.ascontiguousarray(pb, dtype=np.int64).reshape(n, 5)
        pX = np.ascontiguousarray(pX, dtype=np.float32).reshape(n, 5)
        pY = np.ascontiguousarray(pY, dtype=np.float32).reshape(n, 5)
        rr = np.ascontiguousarray(rr, dtype=np.float64).reshape(n, 3)
        params = np.ascontiguousarray(params, dtype=np.float64).reshape(20)
        mk = None if masks is None else np.ascontiguousarray(masks, dtype=np.uint32).reshape(n, 2)
        out = np.zeros(n, dtype=np.float32)
        out64 = np.zeros(n, dtype=np.float64)
        L.check(L.lib().ldw_debug_screen_bound(self._ctx, int(kind), int(na), int(nb), n, L.ptr(g), L.ptr(pa), L.ptr(pb), L.ptr(pX), L.ptr(pY), L.ptr(rr),
                                               L.ptr(mk), L.ptr(params), L.ptr(out), L.ptr(out64)))
        return out64 if kind == 4 else out

    def write_links_tsv(self, which: int, path: str, append: bool = True, nthreads: int = 0):
        """The context's sr (0) / lr (1) table as `pos1 pos2 clust1 clust2 len MI` rows (write.table format); (rows, bytes)."""
        n, nb = C.c_int64(0), C.c_int64(0)
        L.check(L.lib().ldw_write_links_tsv(self._ctx, int(which), str(path).encode(), int(bool(append)), int(nthreads), C.byref(n), C.byref(nb)))
        return int(n.value), int(nb.value)

    def host_trim(self) -> int:
        """Release the host memory the library keeps between calls (writer pool, pinned fetch arena); call between jobs.  Bytes released."""
        n = C.c_int64(0)
        L.check(L.lib().ldw_host_trim(self._ctx, C.byref(n)))
        return int(n.value)

    def lr_stream_begin(self, path: str, append: bool = True, nthreads: int = 0):
        """lr_links.tsv appended while the next ``mi_all_pairs`` runs, item by item (the reference appends per block: R/computePairwiseMI.R:362)."""
        L.check(L.lib().ldw_lr_stream_begin(self._ctx, str(path).encode(), int(bool(append)), int(nthreads)))

    def lr_stream_end(self):
        """Wait for the streaming writer; (rows, bytes, blocks whose rows are in the file)."""
        n, nb, blk = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        L.check(L.lib().ldw_lr_stream_end(self._ctx, C.byref(n), C.byref(nb), C.byref(blk)))
        return int(n.value), int(nb.value), int(blk.value)

    def write_links_tsv_begin(self, which: int, path: str, append: bool = True, nthreads: int = 0):
        """Fetch the table now, derive / format / write it on host threads while the caller goes on (``write_links_tsv_end`` waits)."""
        L.check(L.lib().ldw_write_links_tsv_begin(self._ctx, int(which), str(path).encode(), int(bool(append)), int(nthreads)))

    def write_links_tsv_end(self):
        """(rows, bytes) of the table started by ``write_links_tsv_begin``; raises what its writer reported."""
        n, nb = C.c_int64(0), C.c_int64(0)
        L.check(L.lib().ldw_write_links_tsv_end(self._ctx, C.byref(n), C.byref(nb)))
        return int(n.value), int(nb.value)

    def set_overlap(self, on: bool):
        """GEMM of the next block beside the epilogue/selection of the current one (default on); off = exclusive stage times."""
        L.check(L.lib().ldw_set_overlap(self._ctx, int(bool(on))))

    def set_fused(self, on: bool):
        """Only off is accepted: the fused GEMM + MI epilogue kernel was measured slower and removed (on raises LDW_ERR_STATE)."""
        L.check(L.lib().ldw_set_fused(self._ctx, int(bool(on))))

    def set_mixed(self, on: bool):
        """High-limb block GEMM + gathered low-limb GEMM for the listed units in speculative blocks (default on)."""
        L.check(L.lib().ldw_set_mixed(self._ctx, int(bool(on))))

    def set_path(self, mode: int):
        """Block-wide pass of the speculative blocks: 0 auto (default), 1 limb GEMM paths only, 2 approximate-GEMM path
        (one dual-digit int8 pass + exact class-wise popcount sums of the listed units) or an error."""
        L.check(L.lib().ldw_set_path(self._ctx, int(mode)))

    def set_select(self, mode: int):
        """Long-range selection: 0 auto (sort-free where it applies), 1 always the two radix sorts.  Same tables."""
        L.check(L.lib().ldw_set_select(self._ctx, int(mode)))

    def apx_info(self):
        """Diagnostics of the approximate path for the current weights (after set_weights)."""
        v = np.zeros(6)
        L.check(L.lib().ldw_apx_info(self._ctx, L.ptr(v)))
        return dict(usable=bool(v[0]), delta=float(v[1]), classes=int(v[2]), segments=int(v[3]), transitions=int(v[4]), e_last=int(v[5]))

    def set_screen(self, mode: int):
        """fp32 screen before the fp64 MI evaluation in speculative blocks: 0 off, 1 on (default), 2 verify."""
        L.check(L.lib().ldw_set_screen(self._ctx, int(mode)))

    def set_engine(self, engine: int):
        L.check(L.lib().ldw_set_engine(self._ctx, int(engine)))

    # -- alignment -----------------------------------------------------------
    def reserve(self, L_snps: int, N_seqs: int, max_blk_sz: int = 10000):
        """Start the side thread that creates the pass's streams, pinned staging buffers and code objects (ldw_ctx_reserve) — behind the
        upload of the alignment and the Hamming GEMM instead of inside the first pass.  Optional; set_alignment calls it."""
        L.check(L.lib().ldw_ctx_reserve(self._ctx, int(L_snps), int(N_seqs), int(max_blk_sz)))

    def set_alignment(self, states, max_blk_sz: int = 10000):
        """states: (L, N) uint8 numpy array or CUDA torch tensor (values 0..4)."""
        if _is_torch(states):
            assert states.dtype.__str__() == "torch.uint8" and states.dim() == 2 and states.is_contiguous()
            Ls, Ns = states.shape
            if states.is_cuda:
                # the library reads the tensor on ITS stream: make sure whatever torch stream produced it is done
                import torch
                torch.cuda.synchronize(states.device)
            L.check(L.lib().ldw_set_alignment(self._ctx, L.ptr(states), Ls, Ns, 1 if states.is_cuda else 0))
        else:
            st = L.as_c(states, np.uint8)
            assert st.ndim == 2
            Ls, Ns = st.shape
            L.check(L.lib().ldw_set_alignment(self._ctx, L.ptr(st), Ls, Ns, 0))
        self.L, self.N = int(Ls), int(Ns)
        self._positions = None
        if not getattr(self, "_reserved", False):
            self._reserved = True
            self.reserve(self.L, self.N, max_blk_sz)   # (a side thread: the pinned staging buffers, while the caller goes on to the Hamming weights)

    def alignment_scan(self, chars: np.ndarray) -> np.ndarray:
        """Upload the raw (N, L_total) alignment and return the 5 x L_total allele counts of every column."""
        ch = L.as_c(chars.view(np.uint8) if chars.dtype != np.uint8 else chars, np.uint8)
        out = np.empty((ch.shape[1], 5), dtype=np.int32)
        L.check(L.lib().ldw_alignment_scan(self._ctx, L.ptr(ch), ch.shape[0], ch.shape[1], L.ptr(out)))
        self._scanned = ch.shape
        return np.ascontiguousarray(out.T)

    def fasta_scan(self, path, chunk_rows: int = 0, io_bytes: int = 0, keep_bytes: int = -1):
        """Pass 1 of the native FASTA feeder: stream the (gz) FASTA file through the device counts, one chunk of rows at a time.  Returns
        (names, L_total, 5 x L_total allele counts).  keep_bytes: device bytes the 4-bit packed states may take so that ``fasta_encode``
        does not read the file again (0 never, < 0 automatic)."""
        p = os.fsencode(path)
        n, lt = C.c_int64(), C.c_int64()
        fasta_check(L.lib().ldw_fasta_scan(self._ctx, p, int(chunk_rows), int(io_bytes), int(keep_bytes), C.byref(n), C.byref(lt)), path)
        nb = C.c_int64()
        L.check(L.lib().ldw_fasta_names(self._ctx, None, 0, C.byref(nb)))
        buf = C.create_string_buffer(max(nb.value, 1))
        L.check(L.lib().ldw_fasta_names(self._ctx, buf, nb.value, C.byref(nb)))
        names = [x.decode() for x in buf.raw[:nb.value].split(b"\0")[:-1]]
        self._fasta_n = int(n.value)
        out = np.empty((lt.value, 5), dtype=np.int32)
        L.check(L.lib().ldw_fasta_counts(self._ctx, L.ptr(out)))
        return names, int(lt.value), out.T          # (a view: no second O(L_total) copy on the host)

    def fasta_encode(self, pos: np.ndarray, want_table=True):
        """Pass 2: the 1-based retained columns ``pos`` of the scanned file become the engine's alignment (from the packed copy, or the file
        read again); returns ACGTN_table (5, n_pos)."""
        ps = L.as_c(pos, np.int32)
        tab = np.zeros((len(ps), 5), dtype=np.int32) if want_table else None
        L.check(L.lib().ldw_fasta_encode(self._ctx, L.ptr(ps), len(ps), L.ptr(tab)))
        self.L, self.N = len(ps), self._fasta_n
        return None if tab is None else np.ascontiguousarray(tab.T)

    def encode_alignment(self, chars, pos: np.ndarray, want_table=True, shape=None):
        """chars: (N, L_total) bytes, or None to reuse the alignment kept by ``alignment_scan``; pos: 1-based retained
        columns.  The result becomes the engine's alignment; returns ACGTN_table (5, n_pos)."""
        ps = L.as_c(pos, np.int32)
        tab = np.zeros((len(ps), 5), dtype=np.int32) if want_table else None
        if chars is None:
            n, lt = shape or self._scanned
            L.check(L.lib().ldw_encode_alignment(self._ctx, None, n, lt, L.ptr(ps), len(ps), L.ptr(tab)))
        else:
            ch = L.as_c(chars.view(np.uint8) if chars.dtype != np.uint8 else chars, np.uint8)
            n, lt = ch.shape
            L.check(L.lib().ldw_encode_alignment(self._ctx, L.ptr(ch), n, lt, L.ptr(ps), len(ps), L.ptr(tab)))
        self.L, self.N = len(ps), n
        return None if tab is None else np.ascontiguousarray(tab.T)

    def get_alignment(self) -> np.ndarray:
        out = np.empty((self.L, self.N), dtype=np.uint8)
        L.check(L.lib().ldw_get_alignment(self._ctx, L.ptr(out)))
        return out

    def write_alignment(self, path, snp_idx, names, format: int = 0, append: bool = False, chunk_bytes: int = 0) -> int:
        """The SNP rows ``snp_idx`` (0-based, output column order) of the resident alignment as text, rendered on the device
        (ldw_write_alignment): format 0 FASTA records, 1 the body of write.table's tsv (name, then tab + character per SNP).  ``names``: one
        str per sequence.  Appended or truncating; written in chunks of ``chunk_bytes`` (0: 64 MiB).  Returns the bytes written."""
        idx = L.as_c(snp_idx, np.int32).ravel()
        blob = b"".join(str(n).encode("utf-8") + b"\0" for n in names)
        nb = C.c_int64(0)
        L.check(L.lib().ldw_write_alignment(self._ctx, os.fsencode(path), int(bool(append)), int(format), L.ptr(idx), len(idx), blob, len(blob),
                                            int(chunk_bytes), C.byref(nb)))
        return int(nb.value)

    def annot_snps(self, ref, seg, strand, pos, alt_mask) -> np.ndarray:
        """The coding-effect record of every SNP ``pos`` (1-based) with the A/C/G/T alleles of ``alt_mask`` on the CDS features ``seg`` (nseg x 3:
        lo, hi, feature; each feature's segments contiguous, in coding order) of strands ``strand`` (+1 / -1) over the reference ``ref``
        (uint8 characters), by k_annot_snp (ldw_annot_snps): int32 [n, LDW_ANNOT_REC]."""
        r = L.as_c(ref, np.uint8).ravel()
        sg = L.as_c(seg, np.int32).reshape(-1, 3)
        sd = L.as_c(strand, np.int8).ravel()
        p = L.as_c(pos, np.int32).ravel()
        am = L.as_c(alt_mask, np.uint8).ravel()
        if p.shape != am.shape:
            raise ValueError("pos and alt_mask differ in length")
        out = np.empty((len(p), ANNOT_REC), dtype=np.int32)
        L.check(L.lib().ldw_annot_snps(self._ctx, L.ptr(r), len(r), L.ptr(sg) if len(sg) else None, len(sg), L.ptr(sd) if len(sd) else None, len(sd),
                                       L.ptr(p), L.ptr(am), len(p), L.ptr(out)))
        return out

    def annot_map(self, pos1, pos2, POS):
        """Every link end to its SNP (ldw_annot_map): (SNP index of every annotation row = the distinct link positions ascending, the first
        link end that matches no SNP or several: index into concat(pos1, pos2), or -1).  The rows of the link ends stay on the device."""
        a, b = L.as_c(pos1, np.float64).ravel(), L.as_c(pos2, np.float64).ravel()
        P = L.as_c(POS, np.int32).ravel()
        if a.shape != b.shape:
            raise ValueError("pos1 and pos2 differ in length")
        snp = np.empty(max(len(P), 1), dtype=np.int32)
        rows, bad = C.c_int64(0), C.c_int64(-1)
        L.check(L.lib().ldw_annot_map(self._ctx, L.ptr(a), L.ptr(b), len(a), L.ptr(P), len(P), L.ptr(snp), C.byref(rows), C.byref(bad)))
        return snp[:rows.value].copy(), int(bad.value)

    def annot_links(self, key, aracne, code, cds_id, max_tophits: int):
        """The links of the last ``annot_map`` in order(key, decreasing = TRUE) with the join and detect_top_hits on the device
        (ldw_annot_links): (perm int64, r1 int32, r2 int32, pair int8 = 3 code1 + code2, top int64: sorted indices of the first max_tophits
        top hits)."""
        k, ar = L.as_c(key, np.float64).ravel(), L.as_c(aracne, np.float64).ravel()
        cd, ci = L.as_c(code, np.int8).ravel(), L.as_c(cds_id, np.int32).ravel()
        n = len(k)
        perm, r1, r2 = np.empty(n, np.int64), np.empty(n, np.int32), np.empty(n, np.int32)
        pair, top = np.empty(n, np.int8), np.empty(max(min(int(max_tophits), n), 1), np.int64)
        nt = C.c_int64(0)
        L.check(L.lib().ldw_annot_links(self._ctx, L.ptr(k), L.ptr(ar), n, L.ptr(cd) if len(cd) else None, L.ptr(ci) if len(ci) else None, len(cd),
                                        int(max_tophits), L.ptr(perm), L.ptr(r1), L.ptr(r2), L.ptr(pair), L.ptr(top), C.byref(nt)))
        return perm, r1, r2, pair, top[:nt.value].copy()

    def state_counts(self) -> np.ndarray:
        out = np.empty((self.L, 5), dtype=np.int32)
        L.check(L.lib().ldw_state_counts(self._ctx, L.ptr(out)))
        return np.ascontiguousarray(out.T)  # 5 x L like ACGTN_table

    # -- CDS variation and paint (R/estimateCDSDiversity.R) ----------------------------------------------------
    def cds_variation(self, POS, ref_seq, starts, ends):
        """Per CDS the masked SNP variation per base of the resident alignment (ldw_cds_variation): (var float64 [ncds], NaN where no SNP falls
        inside; snp_var int64 [L]; alt_mask uint8 [L], bit x = state x (A,C,G,T,N) present beside the reference; ref uint8 [L])."""
        ps = L.as_c(POS, np.int32)
        ref = L.as_c(np.frombuffer(ref_seq, dtype=np.uint8) if isinstance(ref_seq, (bytes, bytearray)) else ref_seq, np.uint8)
        st, en = L.as_c(starts, np.int32), L.as_c(ends, np.int32)
        if st.shape != en.shape:
            raise ValueError("starts and ends differ in length")
        var = np.empty(len(st), dtype=np.float64)
        snp_var = np.empty(len(ps), dtype=np.int64)
        alt = np.empty(len(ps), dtype=np.uint8)
        refc = np.empty(len(ps), dtype=np.uint8)
        L.check(L.lib().ldw_cds_variation(self._ctx, L.ptr(ps), len(ps), L.ptr(ref), len(ref), L.ptr(st), L.ptr(en), len(st), L.ptr(var),
                                          L.ptr(snp_var), L.ptr(alt), L.ptr(refc)))
        self._cds_L = len(ps)
        return var, snp_var, alt, refc

    def cds_paint(self, starts, ends, labels, nclust: int, quirk_mode: int = L.QUIRK_REFERENCE):
        """painter over the SNPs of the last ``cds_variation`` (ldw_cds_paint): (paint int32 [L], SNPs left at 0).  ValueError when no SNP lies
        strictly inside a kept CDS."""
        st, en, lb = L.as_c(starts, np.int32), L.as_c(ends, np.int32), L.as_c(labels, np.int32)
        if not (st.shape == en.shape == lb.shape):
            raise ValueError("starts, ends and labels differ in length")
        n0 = C.c_int64(0)
        out = np.empty(getattr(self, "_cds_L", 0), dtype=np.int32)   # (one entry per SNP of the last cds_variation)
        rc = L.lib().ldw_cds_paint(self._ctx, L.ptr(st), L.ptr(en), L.ptr(lb), len(st), int(nclust), int(quirk_mode),
                                   L.ptr(out) if len(out) else None, C.byref(n0))
        if rc == L.LDW_ERR_ARG:
            msg = L.lib().ldw_last_error().decode("utf-8", "replace")
            if "no SNP lies strictly inside" in msg:
                raise ValueError(msg)
        L.check(rc)
        return out, int(n0.value)

    # -- Hamming weights -------------------------------------------------------
    def hamming_weights(self, thresh: int, want_shared=False):
        hdw = np.empty(self.N, dtype=np.float64)
        shared = np.empty((self.N, self.N), dtype=np.int32) if want_shared else None
        L.check(L.lib().ldw_hamming_weights(self._ctx, int(thresh), L.ptr(hdw), L.ptr(shared)))
        return (hdw, shared) if want_shared else hdw

    def nj_tree(self, dist=None):
        """The neighbour-joining tree (ldw_nj_tree) of the resident alignment's Hamming distances, or of ``dist``: a symmetric (n, n)
        float64 matrix with a zero diagonal.  Returns (parent int32 [2n - 2], length float64 [2n - 2]): nodes 0 .. n-1 are the tips, node n + s is made
        by join s, node 2n - 3 is the root (parent -1) with the last three nodes on it; lengths are raw and may be negative.  ``last_timing()`` afterwards, from
        the library's events: ``gemm_ms`` the joins, ``epilogue_ms`` what ran in front of them (upload and checks, or the Hamming GEMM and the fill),
        ``select_ms`` the launches per join, ``total_ms`` the first two together."""
        if dist is None:
            d, n = None, int(self.N)
        else:
            d = L.as_c(dist, np.float64)
            if d.ndim != 2 or d.shape[0] != d.shape[1]:
                raise ValueError(f"dist must be a square matrix, not {d.shape}")
            n = int(d.shape[0])
        m = max(2 * n - 2, 1)
        parent, length = np.empty(m, dtype=np.int32), np.empty(m, dtype=np.float64)
        L.check(L.lib().ldw_nj_tree(self._ctx, L.ptr(d), n, L.ptr(parent), L.ptr(length)))
        return parent, length

    def nj_bootstrap(self, mult, want_trees=False):
        """Bootstrap support of ``nj_tree()`` (ldw_nj_bootstrap).  ``mult``: int32 (B, L), a row per replicate, how often the replicate holds
        each SNP column of the resident alignment (0..63; ``tree.bootstrap_multiplicities`` draws them).  Returns (parent, length, support): the tree of
        ``nj_tree()`` and, int32 [2n - 2], for every join node n .. 2n-4 the number of replicates whose tree has the same split of the tips, -1 at the tips
        and the root; with ``want_trees`` also (rep_parent int32 (B, 2n - 2), rep_length float64 (B, 2n - 2)), the replicates' trees.  ``last_timing()``
        afterwards, summed over the replicates: ``gemm_ms`` the joins, ``epilogue_ms`` digits + GEMMs + fills, ``select_ms`` split sums + look-ups."""
        m = L.as_c(mult, np.int32)
        if m.ndim != 2 or m.shape[1] != self.L:
            raise ValueError(f"mult must be (replicates, {self.L} SNP columns), not {m.shape}")
        B, n = int(m.shape[0]), int(self.N)
        w = max(2 * n - 2, 1)
        parent, length, support = np.empty(w, dtype=np.int32), np.empty(w, dtype=np.float64), np.empty(w, dtype=np.int32)
        rp = np.empty((B, w), dtype=np.int32) if want_trees else None
        rl = np.empty((B, w), dtype=np.float64) if want_trees else None
        # (an empty array has no address to hand over: the library then answers as it does for a null pointer, after its own checks of the state)
        L.check(L.lib().ldw_nj_bootstrap(self._ctx, L.ptr(m) if m.size else None, B, n, L.ptr(parent), L.ptr(length), L.ptr(support), L.ptr(rp), L.ptr(rl)))
        return (parent, length, support, rp, rl) if want_trees else (parent, length, support)

    # -- parsimony on a tree -------------------------------------
    @staticmethod
    def _pars_tree(parent, tip_seq):
        p, t = L.as_c(parent, np.int32).ravel(), L.as_c(tip_seq, np.int32).ravel()
        if len(p) != len(t):
            raise ValueError(f"parent has {len(p)} nodes but tip_seq {len(t)}")
        return p, t, (L.ptr(p) if len(p) else None), (L.ptr(t) if len(t) else None)

    @staticmethod
    def _pairs(pair_a, pair_b):
        """The two SNP lists of K pairs as the C ABI takes them: (a, b, their pointers (None for no pairs), K)."""
        a, b = L.as_c(pair_a, np.int32).ravel(), L.as_c(pair_b, np.int32).ravel()
        if len(a) != len(b):
            raise ValueError(f"{len(a)} first SNPs but {len(b)} second SNPs")
        K = len(a)
        return a, b, (L.ptr(a) if K else None), (L.ptr(b) if K else None), K

    def _pairs_labels(self, pair_a, pair_b, labels, n_clusters):
        """``_pairs`` and the cluster labels of the N sequences: (..., K, lab, its pointer, C), C defaulting to max(labels) + 1."""
        pairs = self._pairs(pair_a, pair_b)
        lab = L.as_c(labels, np.int32).ravel()
        if len(lab) != self.N:
            raise ValueError(f"labels has {len(lab)} entries, the alignment {self.N} sequences")
        if n_clusters is None:
            n_clusters = int(lab.max()) + 1 if len(lab) else 0
        return pairs + (lab, (L.ptr(lab) if len(lab) else None), int(n_clusters))

    def tree_parsimony(self, parent, tip_seq, gap_mode: int = 0):
        """Maximum parsimony of every SNP of the resident alignment on the tree ``parent`` (int32 [nodes], -1 at node 0, ``parent[v] < v``) whose
        childless nodes stand for the sequences ``tip_seq`` (int32 [nodes], -1 at the other nodes): ldw_tree_parsimony.  ``gap_mode`` 0: a tip in state
        N is a wildcard; 1: N is a fifth state.  Returns (score int32 [L], min_changes int32 [L])."""
        p, t, pp, tp = self._pars_tree(parent, tip_seq)
        score, mn = np.empty(max(self.L, 1), dtype=np.int32), np.empty(max(self.L, 1), dtype=np.int32)
        L.check(L.lib().ldw_tree_parsimony(self._ctx, pp, tp, len(p), int(gap_mode), L.ptr(score), L.ptr(mn)))
        return score[:self.L], mn[:self.L]

    def tree_states(self, parent, tip_seq, snp_idx, gap_mode: int = 0) -> np.ndarray:
        """The most-parsimonious reconstruction DESIGN.md 28 states, for the SNPs ``snp_idx`` (0-based, any order, repeats allowed): uint8
        (len(snp_idx), nodes), the state 0..4 of every node (ldw_tree_states)."""
        p, t, pp, tp = self._pars_tree(parent, tip_seq)
        idx = L.as_c(snp_idx, np.int32).ravel()
        out = np.empty((len(idx), len(p)), dtype=np.uint8)
        L.check(L.lib().ldw_tree_states(self._ctx, pp, tp, len(p), int(gap_mode), L.ptr(idx) if len(idx) else None, len(idx), L.ptr(out) if out.size else None))
        return out

    def tree_cochanges(self, parent, tip_seq, pair_a, pair_b, gap_mode: int = 0):
        """For every pair of SNPs (``pair_a[i]``, ``pair_b[i]``): (changes_a, changes_b, co_changes), int32 each — the branches on which each SNP
        changes under that reconstruction, and those on which both do (ldw_tree_cochanges)."""
        p, t, pp, tp = self._pars_tree(parent, tip_seq)
        a, b, pa, pb, K = self._pairs(pair_a, pair_b)
        ca, cb, co = (np.empty(max(K, 1), dtype=np.int32) for _ in range(3))
        L.check(L.lib().ldw_tree_cochanges(self._ctx, pp, tp, len(p), int(gap_mode), pa, pb, K, L.ptr(ca), L.ptr(cb), L.ptr(co)))
        return ca[:K], cb[:K], co[:K]

    # -- the co-change scan ---------------------------------------
    def tree_cochange_scan(self, parent, tip_seq, gap_mode: int = 0, min_changes: int = 2, min_co: int = 2, min_lift: int = 0, min_len: float = -1.0):
        """Over EVERY pair i < j of the SNPs that change on at least ``min_changes`` branches of the tree (ldw_tree_cochange_scan), co the branches on which
        both change: a pair qualifies when co (nodes - 1) >= ``min_lift`` changes[i] changes[j]; with ``min_len`` >= 0 only pairs whose circular distance
        exceeds it take part (needs the SNP meta data).  Returns a dict: ``changes`` int32 (L,) the score of every SNP, ``hist`` uint64 (1024,) the qualifying
        pairs per min(co, 1023), ``best`` int32 (L,) the largest co of every SNP over its qualifying partners (-1: none), ``nge`` int64 (L,) its qualifying
        partners with co >= ``min_co``, ``npairs`` the pairs of the pair set and ``n_qualifying``."""
        p, t, pp, tp = self._pars_tree(parent, tip_seq)
        n = max(self.L, 1)
        changes, best, nge = np.zeros(n, dtype=np.int32), np.full(n, -1, dtype=np.int32), np.zeros(n, dtype=np.int64)
        hist, npairs = np.zeros(1024, dtype=np.uint64), np.zeros(2, dtype=np.int64)
        L.check(L.lib().ldw_tree_cochange_scan(self._ctx, pp, tp, len(p), int(gap_mode), int(min_changes), int(min_co), int(min_lift), float(min_len), L.ptr(changes),
                                               L.ptr(hist), L.ptr(best), L.ptr(nge), L.ptr(npairs)))
        return dict(changes=changes[:self.L], hist=hist, best=best[:self.L], nge=nge[:self.L], npairs=int(npairs[0]), n_qualifying=int(npairs[1]))

    @staticmethod
    def _cochange_lists(cap):
        cap = int(cap)
        return tuple(np.zeros(cap, dtype=np.int32) for _ in range(3)) if cap > 0 else (None, None, None)

    def tree_cochange_links(self, parent, tip_seq, gap_mode: int = 0, min_changes: int = 2, min_co: int = 2, min_lift: int = 0, min_len: float = -1.0, cap: int = 0,
                            best_in=None):
        """The qualifying pairs of ``tree_cochange_scan`` with co >= ``min_co`` (ldw_tree_cochange_links): ``a`` < ``b`` (global, 0-based) and ``co``, in no
        stated order, and ``count``, exact whatever ``cap`` is.  ``cap`` = 0 only counts; a count above ``cap`` raises LdwError LDW_ERR_SIZE, which carries
        the count as ``.count``.  With ``best_in`` (L,) — the ``best`` of a scan with the same arguments — ``partner`` int32 (L,) is the smallest partner of
        every SNP among its qualifying ones with co == best_in, -1 where there is none."""
        p, t, pp, tp = self._pars_tree(parent, tip_seq)
        a, b, co = self._cochange_lists(cap)
        bi = None if best_in is None else L.as_c(best_in, np.int32).reshape(self.L)
        partner = None if bi is None else np.full(max(self.L, 1), -1, dtype=np.int32)
        n = C.c_int64(0)
        try:
            L.check(L.lib().ldw_tree_cochange_links(self._ctx, pp, tp, len(p), int(gap_mode), int(min_changes), int(min_co), int(min_lift), float(min_len), L.ptr(bi),
                                                    max(int(cap), 0), L.ptr(a), L.ptr(b), L.ptr(co), C.byref(n), L.ptr(partner)))
        except L.LdwError as e:
            e.count = int(n.value)
            raise
        k = int(n.value)
        cut = (lambda x: None if x is None else x[:k])
        return dict(a=cut(a), b=cut(b), co=cut(co), count=k, partner=None if partner is None else partner[:self.L])

    @staticmethod
    def _cochange_slots(bits, changes, idx, pos):
        w = L.as_c(bits, np.uint32)
        assert w.ndim == 2, w.shape
        words, M = w.shape
        ch, ix = L.as_c(changes, np.int32).ravel(), L.as_c(idx, np.int32).ravel()
        ps = None if pos is None else L.as_c(pos, np.int32).ravel()
        assert len(ch) == M == len(ix) and (ps is None or len(ps) == M), (w.shape, len(ch), len(ix))
        return w, words, M, ch, ix, ps

    def debug_cochange_scan(self, bits, changes, idx, B, min_co: int = 0, min_lift: int = 0, min_len: float = -1.0, pos=None, g: float = 0.0):
        """The pair kernel of tree_cochange_scan on caller-made bitmaps (ldw_debug_cochange_scan): ``bits`` uint32 (words, M), ``changes`` (M,), ``idx`` (M,)
        the ascending global SNP of every slot, ``B`` the branches; ``pos`` (M,) and ``g`` where ``min_len`` >= 0.  Returns ``hist``, ``best`` (M,), ``nge``
        (M,), ``npairs`` and ``n_qualifying`` over the M slots."""
        w, words, M, ch, ix, ps = self._cochange_slots(bits, changes, idx, pos)
        hist, npairs = np.zeros(1024, dtype=np.uint64), np.zeros(2, dtype=np.int64)
        best, nge = np.full(max(M, 1), -1, dtype=np.int32), np.zeros(max(M, 1), dtype=np.int64)
        L.check(L.lib().ldw_debug_cochange_scan(self._ctx, L.ptr(w), words, M, L.ptr(ch), L.ptr(ix), L.ptr(ps), float(g), int(B), int(min_co), int(min_lift), float(min_len),
                                                L.ptr(hist), L.ptr(best), L.ptr(nge), L.ptr(npairs)))
        return dict(hist=hist, best=best[:M], nge=nge[:M], npairs=int(npairs[0]), n_qualifying=int(npairs[1]))

    def debug_cochange_links(self, bits, changes, idx, B, min_co: int = 0, min_lift: int = 0, min_len: float = -1.0, pos=None, g: float = 0.0, cap: int = 0, best_in=None):
        """The pair kernel of tree_cochange_links on caller-made bitmaps (ldw_debug_cochange_links), as debug_cochange_scan: the dict of tree_cochange_links
        over the M slots (``a`` / ``b`` and ``partner`` are global SNPs from ``idx``)."""
        w, words, M, ch, ix, ps = self._cochange_slots(bits, changes, idx, pos)
        a, b, co = self._cochange_lists(cap)
        bi = partner = None
        if best_in is not None:          # (one entry at least: an empty array has no pointer to give)
            bi, partner = np.full(max(M, 1), -1, dtype=np.int32), np.full(max(M, 1), -1, dtype=np.int32)
            bi[:M] = L.as_c(best_in, np.int32).reshape(M)
        n = C.c_int64(0)
        try:
            L.check(L.lib().ldw_debug_cochange_links(self._ctx, L.ptr(w), words, M, L.ptr(ch), L.ptr(ix), L.ptr(ps), float(g), int(B), int(min_co), int(min_lift),
                                                     float(min_len), L.ptr(bi), max(int(cap), 0), L.ptr(a), L.ptr(b), L.ptr(co), C.byref(n), L.ptr(partner)))
        except L.LdwError as e:
            e.count = int(n.value)
            raise
        k = int(n.value)
        cut = (lambda x: None if x is None else x[:k])
        return dict(a=cut(a), b=cut(b), co=cut(co), count=k, partner=None if partner is None else partner[:M])

    # -- the lineage check ---------------------------------------
    def seq_clusters(self, thresh):
        """Single-linkage clusters of the resident alignment's sequences (ldw_seq_clusters): i and j are neighbours iff they differ in fewer than
        ``thresh`` SNP columns.  ``thresh``: an int, or up to 16 of them served from one Hamming GEMM.  Returns (labels, n_clusters): int32 [N] and an
        int for one threshold, int32 (n_thresh, N) and int32 [n_thresh] for a sequence; clusters are numbered in the order of their smallest member.
        ``last_timing()`` afterwards: ``gemm_ms`` the rounds, ``epilogue_ms`` what ran in front of them, ``select_ms`` the rounds taken."""
        one = np.ndim(thresh) == 0
        th = L.as_c(np.atleast_1d(thresh), np.int32).ravel()
        labels = np.empty((max(len(th), 1), max(self.N, 1)), dtype=np.int32)
        n = np.empty(max(len(th), 1), dtype=np.int32)
        L.check(L.lib().ldw_seq_clusters(self._ctx, L.ptr(th) if len(th) else None, len(th), L.ptr(labels), L.ptr(n)))
        labels, n = labels[:len(th), :self.N], n[:len(th)]
        return (labels[0], int(n[0])) if one else (labels, n)

    def links_stratified(self, pair_a, pair_b, labels, C=None, want_tables=False):
        """Per cluster of ``labels`` (int [N]: 0 .. C-1, or -1 for a sequence left out; ``C`` defaults to max(labels) + 1) the weighted MI of the SNP
        pairs (``pair_a[i]``, ``pair_b[i]``) over the cluster's members alone, under the resident weights (ldw_links_stratified).  Returns a dict:
        ``mi`` float64 (K, C), ``mi_all`` float64 [K] (over all labelled sequences), ``poly`` uint8 (K, C) (bit 0: the first SNP is polymorphic in the
        cluster, bit 1: the second), ``neff`` float64 [C], ``frac_bits``; with ``want_tables`` also ``counts`` and ``fixed``, int64 (K, C, 5, 5)."""
        a, b, pa, pb, K, lab, plab, C = self._pairs_labels(pair_a, pair_b, labels, C)
        shape = (max(K, 1), max(min(C, 65536), 1))
        mi, mi_all, poly = np.empty(shape), np.empty(shape[0]), np.empty(shape, dtype=np.uint8)
        neff = np.empty(shape[1])
        cnt = np.empty(shape + (5, 5), dtype=np.int64) if want_tables else None
        fix = np.empty(shape + (5, 5), dtype=np.int64) if want_tables else None
        fb = c_int(0)
        L.check(L.lib().ldw_links_stratified(self._ctx, pa, pb, K, plab, C, L.ptr(mi), L.ptr(mi_all), L.ptr(poly), L.ptr(neff), L.ptr(cnt), L.ptr(fix), byref(fb)))
        out = dict(mi=mi, mi_all=mi_all, poly=poly, neff=neff, frac_bits=fb.value)
        if want_tables:
            out.update(counts=cnt, fixed=fix)
        return out

    # -- the permutation test -------------------------------------
    def links_permuted(self, pair_a, pair_b, labels, n_perm, seed=0, C=None, want_null=False, want_tables=False, want_orders=False):
        """The weighted MI of the SNP pairs (``pair_a[i]``, ``pair_b[i]``) over the labelled sequences and its null distribution under ``n_perm``
        permutations of the second SNP's states among the sequences of every cluster of ``labels`` (as ``links_stratified`` takes them; ``C`` defaults
        to max(labels) + 1), under the resident weights (ldw_links_permuted).  Returns a dict: ``mi_obs`` float64 [K] (bit-equal to
        ``links_stratified(...)["mi_all"]``), ``n_ge`` int32 [K] (replicates whose MI reaches the observed one), ``null_max`` float64 [K], ``P`` (the
        labelled sequences), ``n_perm``, ``frac_bits``; with ``want_null`` also ``null`` float64 (K, n_perm), with ``want_tables`` ``fixed`` int64
        (K, n_perm, 5, 5), with ``want_orders`` ``orders`` int32 (n_perm, P).  A replicate is a function of (labels, seed, its number) alone."""
        a, b, pa, pb, K, lab, plab, C = self._pairs_labels(pair_a, pair_b, labels, C)
        B = int(n_perm)
        seed = int(seed)
        if not 0 <= seed < 1 << 64:
            raise ValueError(f"seed {seed} is not an unsigned 64-bit integer")
        if not -(1 << 31) <= B < 1 << 31:
            raise ValueError(f"n_perm {B} is out of range")
        rows, reps, n_lab = max(K, 1), max(min(B, 1 << 24), 1), max(int((lab >= 0).sum()), 1)
        mi_obs, n_ge, null_max = np.empty(rows), np.empty(rows, dtype=np.int32), np.empty(rows)
        null = np.empty((rows, reps)) if want_null else None
        fix = np.empty((rows, reps, 5, 5), dtype=np.int64) if want_tables else None
        orders = np.empty((reps, n_lab), dtype=np.int32) if want_orders else None
        p_out, fb = c_int64(0), c_int(0)
        L.check(L.lib().ldw_links_permuted(self._ctx, pa, pb, K, plab, C, B, seed, L.ptr(mi_obs), L.ptr(n_ge), L.ptr(null_max), L.ptr(null), L.ptr(fix),
                                           L.ptr(orders), byref(p_out), byref(fb)))
        out = dict(mi_obs=mi_obs, n_ge=n_ge, null_max=null_max, P=int(p_out.value), n_perm=B, frac_bits=fb.value)
        if want_null:
            out["null"] = null
        if want_tables:
            out["fixed"] = fix
        if want_orders:
            out["orders"] = orders
        return out

    def hamming_counts(self, thresh: int, tile0: int, tile1: int) -> np.ndarray:
        """Contribution of the strip of 128-sequence row tiles [tile0, tile1) to the neighbour counts n_j (all j)."""
        out = np.zeros(self.N, dtype=np.int64)
        L.check(L.lib().ldw_hamming_counts(self._ctx, int(thresh), int(tile0), int(tile1), L.ptr(out)))
        return out

    # -- MI --------------------------------------------------------------------
    def set_weights(self, hdw, nlimbs: int = 0):
        w = L.as_c(hdw, np.float64)
        L.check(L.lib().ldw_set_weights(self._ctx, L.ptr(w), len(w), int(nlimbs)))

    def set_snp_meta(self, r, uqe, POS, paint, g):
        r_ = L.as_c(r, np.float64)
        uq = L.as_c(np.asarray(uqe) != 0, np.uint8)
        ps = L.as_c(POS, np.int32)
        pt = None if paint is None else L.as_c(paint, np.int32)
        assert r_.shape == (self.L,) and uq.shape == (self.L, 5) and ps.shape == (self.L,)
        L.check(L.lib().ldw_set_snp_meta(self._ctx, L.ptr(r_), L.ptr(uq), L.ptr(ps), L.ptr(pt), float(g)))
        self._positions = ps

    def mi_block(self, from_idx, to_idx, quirk=L.QUIRK_REFERENCE, out=None) -> np.ndarray:
        """MI of one block as the reference's nf x nt matrix (Fortran order)."""
        fi = L.as_c(from_idx, np.int32)
        ti = L.as_c(to_idx, np.int32)
        if out is not None and _is_torch(out):
            L.check(L.lib().ldw_mi_block(self._ctx, L.ptr(fi), len(fi), L.ptr(ti), len(ti), quirk, L.ptr(out), 1))
            return out
        buf = np.empty(len(fi) * len(ti), dtype=np.float64)
        L.check(L.lib().ldw_mi_block(self._ctx, L.ptr(fi), len(fi), L.ptr(ti), len(ti), quirk, L.ptr(buf), 0))
        return buf.reshape((len(fi), len(ti)), order="F")

    def joint_tables(self, pair_a, pair_b):
        """(counts, fixed, frac_bits): int64 (P,5,5) unweighted joint counts and fixed-point weighted sums."""
        pa = L.as_c(pair_a, np.int32)
        pb = L.as_c(pair_b, np.int32)
        cnt = np.empty((len(pa), 5, 5), dtype=np.int64)
        fix = np.empty((len(pa), 5, 5), dtype=np.int64)
        fb = C.c_int(0)
        L.check(L.lib().ldw_joint_tables(self._ctx, L.ptr(pa), L.ptr(pb), len(pa), L.ptr(cnt), L.ptr(fix), C.byref(fb)))
        return cnt, fix, fb.value

    def mi_all_pairs(self, blocks, sr_dist=20000.0, lr_retain_links=1e6, lr_links_approx=1.0, sr_only=False,
                     quirk=L.QUIRK_REFERENCE, keep_sr=True):
        """blocks: (nb, 4) int32 rows (from_s, from_e, to_s, to_e), 1-based inclusive."""
        bl = L.as_c(blocks, np.int32).reshape(-1, 4)
        p = L.MIParams(float(sr_dist), float(lr_retain_links), float(lr_links_approx), int(bool(sr_only)), int(quirk),
                       int(bool(keep_sr)), 0)
        L.check(L.lib().ldw_mi_all_pairs(self._ctx, L.ptr(bl), len(bl), C.byref(p), 1))
        self._nblocks = len(bl)

    @staticmethod
    def mi_all_pairs_multi(engines, blocks, sr_dist=20000.0, lr_retain_links=1e6, lr_links_approx=1.0, sr_only=False,
                           quirk=L.QUIRK_REFERENCE, keep_sr=True, sr_rows_stay=False):
        """The block loop over several engines of THIS process, one per GPU (ldw_mi_all_pairs_multi): every engine must hold the same
        alignment, weights and SNP meta data; the blocks are dealt by cost, each engine runs its share on a worker thread inside the
        library, and engines[0] ends up with the assembled tables in make_blocks order (and the block statistics of all blocks) — exactly
        as if it had run every block itself.  Returns dict(owner=int32[nblocks], pass_ms, gather_ms, per_engine_ms).
        ``sr_rows_stay`` (LDW_MI_SR_ROWS_STAY): only the long-range table is assembled; every engine keeps the short-range rows of its own
        share and ``EngineGroup(engines)`` runs the short-range model over them."""
        bl = L.as_c(blocks, np.int32).reshape(-1, 4)
        p = L.MIParams(float(sr_dist), float(lr_retain_links), float(lr_links_approx), int(bool(sr_only)), int(quirk),
                       int(bool(keep_sr)), L.MI_SR_ROWS_STAY if sr_rows_stay else 0)
        arr = (C.c_void_p * len(engines))(*[e._ctx.value for e in engines])
        owner = np.zeros(len(bl), dtype=np.int32)
        ms = np.zeros(10, dtype=np.float64)
        L.check(L.lib().ldw_mi_all_pairs_multi(arr, len(engines), L.ptr(bl), len(bl), C.byref(p), L.ptr(owner), L.ptr(ms)))
        engines[0]._nblocks = len(bl)
        for k, e in enumerate(engines[1:], start=1):
            e._nblocks = int((owner == k).sum())
        return dict(owner=owner, pass_ms=float(ms[0]), gather_ms=float(ms[1]), per_engine_ms=ms[2:2 + min(len(engines), 8)].tolist())

    @staticmethod
    def hamming_weights_multi(engines, thresh: int) -> np.ndarray:
        """estimate_Hamming_distance_weights with the sequence x sequence comparison cut into one strip per engine (same alignment on all)."""
        arr = (C.c_void_p * len(engines))(*[e._ctx.value for e in engines])
        hdw = np.empty(engines[0].N, dtype=np.float64)
        L.check(L.lib().ldw_hamming_weights_multi(arr, len(engines), int(thresh), L.ptr(hdw)))
        return hdw

    def links_begin(self, nblocks: int):
        L.check(L.lib().ldw_links_begin(self._ctx, int(nblocks)))
        self._nblocks = 0

    def mi_block_links(self, from_idx, to_idx, sr_dist=20000.0, lr_retain_links=1e6, lr_links_approx=1.0, sr_only=False,
                       quirk=L.QUIRK_REFERENCE, keep_sr=True):
        fi = L.as_c(from_idx, np.int32)
        ti = L.as_c(to_idx, np.int32)
        p = L.MIParams(float(sr_dist), float(lr_retain_links), float(lr_links_approx), int(bool(sr_only)), int(quirk),
                       int(bool(keep_sr)), 0)
        L.check(L.lib().ldw_mi_block_links(self._ctx, L.ptr(fi), len(fi), L.ptr(ti), len(ti), C.byref(p)))
        self._nblocks += 1

    def links_end(self):
        L.check(L.lib().ldw_links_end(self._ctx))

    def links_count(self, which: int) -> int:
        n = C.c_int64(0)
        L.check(L.lib().ldw_links_count(self._ctx, int(which), C.byref(n)))
        return int(n.value)

    def links_view(self, which: int):
        """(a, b, MI) as torch tensors that ALIAS the context's own table in HBM (no copy): valid until the next call that
        changes the table; do not write to them.  STREAM ORDER: the library writes its tables from its own streams, so any
        asynchronous torch read of these views (a cat, a send) must have COMPLETED — synchronise the torch stream that reads —
        before the next ldw_mi_all_pairs / ldw_links_begin / ldw_links_import on this engine (dist.gather_begin does)."""
        import torch
        pa, pb, pm, n = C.c_void_p(0), C.c_void_p(0), C.c_void_p(0), C.c_int64(0)
        L.check(L.lib().ldw_links_device_ptrs(self._ctx, int(which), C.byref(pa), C.byref(pb), C.byref(pm), C.byref(n)))

        class _View:
            def __init__(self, ptr, n, typestr):
                self.__cuda_array_interface__ = dict(shape=(n,), typestr=typestr, data=(ptr or 0, False), version=2)

        dev = torch.device("cuda", self.device)
        if n.value == 0:
            return torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.float64, device=dev)
        mk = lambda p, ts: torch.as_tensor(_View(p.value, n.value, ts), device=dev)
        return mk(pa, "<i4"), mk(pb, "<i4"), mk(pm, "<f8")

    def links(self, which: int, device_tensors=False):
        """(a, b, MI): 0-based from-side / to-side SNP indices and MI of the short-range (0) or long-range (1) table."""
        n = self.links_count(which)
        if device_tensors:
            import torch
            dev = torch.device("cuda", self.device)
            a = torch.empty(n, dtype=torch.int32, device=dev)
            b = torch.empty(n, dtype=torch.int32, device=dev)
            mi = torch.empty(n, dtype=torch.float64, device=dev)
            L.check(L.lib().ldw_links_fetch(self._ctx, which, L.ptr(a), L.ptr(b), L.ptr(mi), n, 1))
            return a, b, mi
        a = np.empty(n, dtype=np.int32)
        b = np.empty(n, dtype=np.int32)
        mi = np.empty(n, dtype=np.float64)
        L.check(L.lib().ldw_links_fetch(self._ctx, which, L.ptr(a), L.ptr(b), L.ptr(mi), n, 0))
        return a, b, mi

    def links_import(self, which: int, a, b, mi):
        """Replace the context's sr (0) / lr (1) table, e.g. by the table assembled from all ranks (dist.gather_link_tables)."""
        if _is_torch(a):
            a, b, mi = a.contiguous(), b.contiguous(), mi.contiguous()
            assert a.dtype.__str__() == "torch.int32" and mi.dtype.__str__() == "torch.float64" and len(a) == len(b) == len(mi)
            on_dev = int(a.is_cuda)
            if on_dev:   # the library copies on its own (non-blocking) stream: torch's producers (cat, RCCL receives) must be done
                import torch
                torch.cuda.synchronize(a.device)
        else:
            a, b, mi = np.ascontiguousarray(a, dtype=np.int32), np.ascontiguousarray(b, dtype=np.int32), np.ascontiguousarray(mi, dtype=np.float64)
            on_dev = 0
        L.check(L.lib().ldw_links_import(self._ctx, int(which), L.ptr(a), L.ptr(b), L.ptr(mi), len(mi), on_dev))

    # -- link tables from files (include/ldweaver_amd.h 13) ------------------------
    def tsv_read(self, path, sep: str, ncols: int, chunk_bytes: int = 0):
        """Parse a numeric table (plain or gzip, no header, one separator byte) into the context's device columns (ldw_tsv_read).
        Returns (rows, slow cells, tuple of per-column "every cell was a plain integer literal")."""
        rows, slow, mask = C.c_int64(0), C.c_int64(0), C.c_uint32(0)
        fasta_check(L.lib().ldw_tsv_read(self._ctx, os.fsencode(path), ord(sep), int(ncols), int(chunk_bytes), C.byref(rows), C.byref(slow), C.byref(mask)), path)
        return rows.value, slow.value, tuple(bool(mask.value >> k & 1) for k in range(int(ncols)))

    def tsv_columns(self):
        """The columns of the last tsv_read as float64 torch tensors that ALIAS the context's buffer (no copy): valid until the next tsv_read or
        close(); read-only.  The stream order of ``links_view`` applies."""
        import torch
        p, rows, ncols, stride = C.c_void_p(0), C.c_int64(0), C.c_int32(0), C.c_int64(0)
        L.check(L.lib().ldw_tsv_columns(self._ctx, C.byref(p), C.byref(rows), C.byref(ncols), C.byref(stride)))
        dev = torch.device("cuda", self.device)
        if rows.value == 0:
            return [torch.empty(0, dtype=torch.float64, device=dev) for _ in range(ncols.value)]

        class _View:
            def __init__(self, ptr, n):
                self.__cuda_array_interface__ = dict(shape=(n,), typestr="<f8", data=(ptr, False), version=2)

        return [torch.as_tensor(_View(p.value + 8 * stride.value * k, rows.value), device=dev) for k in range(ncols.value)]

    def tsv_fetch(self, col: int, rows: int) -> np.ndarray:
        out = np.empty(int(rows), dtype=np.float64)
        L.check(L.lib().ldw_tsv_fetch(self._ctx, int(col), L.ptr(out), len(out), 0))
        return out

    def tsv_stats(self) -> dict:
        v = np.zeros(10)
        L.check(L.lib().ldw_tsv_stats(self._ctx, L.ptr(v)))
        return dict(total_ms=v[0], read_ms=v[1], copy_ms=v[2], line_ms=v[3], parse_ms=v[4], patch_ms=v[5], chunks=int(v[6]), bytes=int(v[7]), grows=int(v[8]),
                    pinned_bytes=int(v[9]))

    # -- annotated link files searched on the device (include/ldweaver_amd.h 14) ---
    def links_grep(self, path, needles, drop_syXsy: bool = False, drop_indirect: bool = False, chunk_bytes: int = 0) -> dict:
        """The rows of an annotated link file (sr_links_annotated.tsv / lr_links_annotated.tsv) whose pos1_ann or pos2_ann field holds one of
        ``needles`` (bytes or str, literal and case sensitive), in file order (ldw_links_grep + ldw_links_grep_fetch).  Returns a dict: ``row``
        (int64, 0-based data row), ``num`` (float64 [rows, 5]: pos1 pos2 len ARACNE MI), ``mask`` (uint64 [rows, ceil(n / 64)]), ``pos1_ann`` /
        ``pos2_ann`` / ``links`` (lists of bytes), ``data_rows`` (rows of the file)."""
        nd = [x.encode("utf-8", "surrogateescape") if isinstance(x, str) else bytes(x) for x in needles]
        off = np.zeros(len(nd) + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(x) for x in nd])
        blob = np.frombuffer(b"".join(nd) or b"\0", dtype=np.uint8)
        flags = (1 if drop_syXsy else 0) | (2 if drop_indirect else 0)
        rows, tbytes, drows = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        fasta_check(L.lib().ldw_links_grep(self._ctx, os.fsencode(path), L.ptr(blob), L.ptr(off), len(nd), flags, int(chunk_bytes), C.byref(rows), C.byref(tbytes),
                                           C.byref(drows)), path)
        n, nw = rows.value, (len(nd) + 63) // 64
        row = np.empty(n, dtype=np.int64)
        num = np.empty((n, 5), dtype=np.float64)
        mask = np.empty((n, nw), dtype=np.uint64)
        text = np.empty(max(tbytes.value, 1), dtype=np.uint8)
        toff = np.empty(3 * n + 1, dtype=np.int64)
        L.check(L.lib().ldw_links_grep_fetch(self._ctx, n, tbytes.value, L.ptr(row), L.ptr(num), L.ptr(mask), L.ptr(text), L.ptr(toff)))
        tb = text.tobytes()
        strs = [tb[toff[k]:toff[k + 1]] for k in range(3 * n)]
        return dict(row=row, num=num, mask=mask, pos1_ann=strs[0::3], pos2_ann=strs[1::3], links=strs[2::3], data_rows=drows.value)

    def links_grep_stats(self) -> dict:
        v = np.zeros(8)
        L.check(L.lib().ldw_links_grep_stats(self._ctx, L.ptr(v)))
        return dict(total_ms=v[0], read_ms=v[1], copy_ms=v[2], line_ms=v[3], grep_ms=v[4], chunks=int(v[5]), bytes=int(v[6]), kept=int(v[7]))

    # -- the network plot (include/ldweaver_amd.h 12) --------------------------------
    @staticmethod
    def _c_strings(seq):
        """The labels of a figure, encoded, and the ``char *`` array over them (one entry at least; the list keeps the bytes alive)."""
        names = [x.encode("utf-8", "replace") if isinstance(x, str) else bytes(x) for x in seq]
        return names, (C.c_char_p * max(len(names), 1))(*names)

    CAPSULE = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("w", "<i4"), ("rgb", "<u4"), ("alpha", "<i4")])

    def plot_capsules(self, caps, W: int, H: int, timings: bool = False):
        """The raw raster of a capsule list (ldw_debug_plot_capsules): uint8 [H, W, 3]; with ``timings`` also (binning ms, shading ms)."""
        caps = np.ascontiguousarray(caps, dtype=self.CAPSULE)
        out = np.empty((int(H), int(W), 3), dtype=np.uint8)
        ms = np.zeros(2)
        L.check(L.lib().ldw_debug_plot_capsules(self._ctx, L.ptr(caps) if len(caps) else None, len(caps), int(W), int(H), L.ptr(out), L.ptr(ms) if timings else None))
        return (out, tuple(ms)) if timings else out

    def plot_network(self, caps, W: int, H: int, node_xy, node_names, title, legend_value, legend_rgb, text_scale: int, png_path=None, want_canvas: bool = False):
        """The network figure (ldw_plot_network).  Returns (canvas uint8 [H, W, 3] or None, boxes int32 [nodes + 2, 4])."""
        caps = np.ascontiguousarray(caps, dtype=self.CAPSULE)
        xy = np.ascontiguousarray(node_xy, dtype=np.int32).reshape(-1, 2)
        names, arr = self._c_strings(node_names)
        lv = np.ascontiguousarray(legend_value, dtype=np.int32)
        lc = np.ascontiguousarray(legend_rgb, dtype=np.uint32)
        boxes = np.zeros((len(names) + 2, 4), dtype=np.int32)
        canvas = np.empty((int(H), int(W), 3), dtype=np.uint8) if want_canvas else None
        L.check(L.lib().ldw_plot_network(self._ctx, L.ptr(caps) if len(caps) else None, len(caps), int(W), int(H), L.ptr(xy) if len(names) else None,
                                         C.cast(arr, C.c_void_p) if len(names) else None, len(names), (title or "").encode("utf-8", "replace"),
                                         L.ptr(lv) if len(lv) else None, L.ptr(lc) if len(lc) else None, len(lv), int(text_scale),
                                         os.fsencode(png_path) if png_path is not None else None, L.ptr(canvas), L.ptr(boxes)))
        return canvas, boxes

    # -- the tanglegram (include/ldweaver_amd.h 12) ------------------------------------
    RECT = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("rgb", "<u4")])

    def debug_plot_marks(self, caps, rects, W: int, H: int, timings: bool = False):
        """The raw raster of a tanglegram's marks (ldw_debug_plot_marks): the capsules, then the opaque half-open rectangles (structured ``Engine.RECT``
        array) in list order: uint8 [H, W, 3]; with ``timings`` also (binning, shading, rectangles) in ms."""
        caps = np.ascontiguousarray(caps, dtype=self.CAPSULE)
        rects = np.ascontiguousarray(rects, dtype=self.RECT)
        out = np.empty((int(H), int(W), 3), dtype=np.uint8)
        ms = np.zeros(3)
        L.check(L.lib().ldw_debug_plot_marks(self._ctx, L.ptr(caps) if len(caps) else None, len(caps), L.ptr(rects) if len(rects) else None, len(rects), int(W),
                                             int(H), L.ptr(out), L.ptr(ms) if timings else None))
        return (out, tuple(ms)) if timings else out

    def plot_tanglegram(self, caps, rects, W: int, H: int, label_xy, labels, title, text_scale: int, png_path=None, want_canvas: bool = False):
        """The tanglegram figure (ldw_plot_tanglegram): labels read upwards from their anchors.  Returns (canvas uint8 [H, W, 3] or None, boxes int32
        [labels + 1, 4]: the labels, the title)."""
        caps = np.ascontiguousarray(caps, dtype=self.CAPSULE)
        rects = np.ascontiguousarray(rects, dtype=self.RECT)
        xy = np.ascontiguousarray(label_xy, dtype=np.int32).reshape(-1, 2)
        names, arr = self._c_strings(labels)
        if len(names) != len(xy):
            raise ValueError(f"{len(names)} labels for {len(xy)} anchors")
        boxes = np.zeros((len(names) + 1, 4), dtype=np.int32)
        canvas = np.empty((int(H), int(W), 3), dtype=np.uint8) if want_canvas else None
        L.check(L.lib().ldw_plot_tanglegram(self._ctx, L.ptr(caps) if len(caps) else None, len(caps), L.ptr(rects) if len(rects) else None, len(rects), int(W),
                                            int(H), L.ptr(xy) if len(names) else None, C.cast(arr, C.c_void_p) if len(names) else None, len(names),
                                            (title or "").encode("utf-8", "replace"), int(text_scale), os.fsencode(png_path) if png_path is not None else None,
                                            L.ptr(canvas), L.ptr(boxes)))
        return canvas, boxes

    # -- the tree view (include/ldweaver_amd.h 15) ------------------------------------
    BAR = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4")])

    def _tree_args(self, W, H, panel, bars, bar_rgb, levels, palette, band_rect):
        bars = np.ascontiguousarray(bars, dtype=self.BAR)
        panel = np.ascontiguousarray(panel, dtype=np.int32).reshape(4)
        rect = np.ascontiguousarray(band_rect if band_rect is not None else np.zeros((0, 4)), dtype=np.int32).reshape(-1, 4)
        R = len(rect)
        lev = np.ascontiguousarray(levels if levels is not None else np.zeros((0, 1)), dtype=np.uint8).reshape(R, -1) if R else np.zeros((0, 0), dtype=np.uint8)
        pal = np.ascontiguousarray(palette if palette is not None else np.zeros((0, 256)), dtype=np.uint32).reshape(R, 256) if R else np.zeros((0, 256), dtype=np.uint32)
        keep = (bars, panel, rect, lev, pal)
        args = (int(W), int(H), L.ptr(panel), L.ptr(bars) if len(bars) else None, len(bars), int(bar_rgb), L.ptr(lev) if R else None, lev.shape[1] if R else 0,
                L.ptr(pal) if R else None, L.ptr(rect) if R else None, R)
        return keep, args

    def plot_tree_raster(self, W: int, H: int, panel, bars, bar_rgb: int = 0, levels=None, palette=None, band_rect=None, timings: bool = False):
        """The raw canvas of the tree view (ldw_debug_plot_tree): uint8 [H, W, 3]: white, the bars (structured ``Engine.BAR`` array, 1/16 pixel relative
        to ``panel`` = x, y, w, h) and the bands (``levels`` uint8 [bands, tips], ``palette`` uint32 [bands, 256], ``band_rect`` int32 [bands, 4]);
        with ``timings`` also (clear, bars, bands, colour) in ms."""
        keep, args = self._tree_args(W, H, panel, bars, bar_rgb, levels, palette, band_rect)
        out = np.empty((int(H), int(W), 3), dtype=np.uint8)
        ms = np.zeros(4)
        L.check(L.lib().ldw_debug_plot_tree(self._ctx, *args, L.ptr(out), L.ptr(ms) if timings else None))
        return (out, tuple(ms)) if timings else out

    def plot_tree(self, W: int, H: int, panel, bars, bar_rgb: int = 0, levels=None, palette=None, band_rect=None, band_labels=None, title=None, legends=(),
                  text_scale: int = 1, png_path=None, want_canvas: bool = False):
        """The tree figure (ldw_plot_tree).  ``legends``: up to two of (title, labels, colours 0xRRGGBB, (x, y)).  Returns (canvas uint8 [H, W, 3] or
        None, boxes int32 [bands + 3, 4]: the band labels, the title, the two legends)."""
        keep, args = self._tree_args(W, H, panel, bars, bar_rgb, levels, palette, band_rect)
        R = args[-1]
        labels, lab_arr = self._c_strings(band_labels if band_labels is not None else [""] * R)
        if len(labels) != R:
            raise ValueError(f"{len(labels)} band labels for {R} bands")
        legends = list(legends) + [("", [], [], (0, 0))] * (2 - len(legends))
        if len(legends) != 2:
            raise ValueError("at most two legends")
        _, lt = self._c_strings([g[0] for g in legends])
        ln = np.asarray([len(g[1]) for g in legends], dtype=np.int32)
        entries, le = self._c_strings([s for g in legends for s in g[1]])
        lc = np.ascontiguousarray([int(v) for g in legends for v in g[2]], dtype=np.uint32)
        if len(lc) != len(entries):
            raise ValueError("a legend needs one colour per label")
        lxy = np.ascontiguousarray([v for g in legends for v in g[3]], dtype=np.int32).reshape(4)
        boxes = np.zeros((R + 3, 4), dtype=np.int32)
        canvas = np.empty((int(H), int(W), 3), dtype=np.uint8) if want_canvas else None
        L.check(L.lib().ldw_plot_tree(self._ctx, *args, C.cast(lab_arr, C.c_void_p) if R else None, self._c_strings([title or ""])[0][0], C.cast(lt, C.c_void_p), L.ptr(ln),
                                      C.cast(le, C.c_void_p) if entries else None, L.ptr(lc) if entries else None, L.ptr(lxy), int(text_scale),
                                      os.fsencode(png_path) if png_path is not None else None, L.ptr(canvas), L.ptr(boxes)))
        return canvas, boxes

    def set_positions(self, POS, g: float = 0.0):
        """Positions for an engine WITHOUT an alignment (ldw_set_positions): enough for links_load / links_import, ldmap, lr_tukey, lr_reduced,
        aracne_device and the long-range figure; g = 0: genome length not known."""
        ps = L.as_c(POS, np.int32)
        assert ps.ndim == 1
        L.check(L.lib().ldw_set_positions(self._ctx, L.ptr(ps), len(ps), float(g)))
        self.L, self.N = len(ps), 0
        self._positions = ps

    def links_load(self, which: int, pos1_col: int, pos2_col: int, mi_col: int, min_len_col: int = -1, min_len: float = 0.0) -> int:
        """The columns of the last tsv_read become the sr (0) / lr (1) table, on the device (ldw_links_load).  Returns the rows installed."""
        n = C.c_int64(0)
        L.check(L.lib().ldw_links_load(self._ctx, int(which), int(pos1_col), int(pos2_col), int(mi_col), int(min_len_col), float(min_len), 0, C.byref(n)))
        return n.value

    def block_stats(self):
        nb = self._nblocks
        t = np.empty(nb, dtype=np.int64)
        k = np.empty(nb, dtype=np.int64)
        s = np.empty(nb, dtype=np.int64)
        d = np.empty(nb, dtype=np.float64)
        L.check(L.lib().ldw_block_stats(self._ctx, nb, L.ptr(t), L.ptr(k), L.ptr(s), L.ptr(d)))
        return dict(n_lr_total=t, n_lr_kept=k, n_sr=s, disc_thresh=d)

    # -- short-range model / ARACNE on the device-resident sr table ---------------
    def sr_len_quantiles(self, nclust: int, sr_dist: float, prob: float = 0.95):
        """(q_lo, q_hi, n), each (nclust, S) with S = ceil(sr_dist)-1; column l-1 is len l."""
        S = int(np.ceil(sr_dist)) - 1
        qlo = np.empty((nclust, S), dtype=np.float64)
        qhi = np.empty((nclust, S), dtype=np.float64)
        n = np.empty((nclust, S), dtype=np.int64)
        L.check(L.lib().ldw_sr_len_quantiles(self._ctx, int(nclust), float(sr_dist), float(prob), S, L.ptr(qlo), L.ptr(qhi), L.ptr(n)))
        return qlo, qhi, n

    def sr_excess_stats(self, mean_dist: np.ndarray) -> np.ndarray:
        md = np.ascontiguousarray(mean_dist, dtype=np.float64)
        out = np.empty((md.shape[0], 5), dtype=np.float64)
        L.check(L.lib().ldw_sr_excess_stats(self._ctx, md.shape[0], md.shape[1], L.ptr(md), L.ptr(out)))
        return out

    def sr_pvalues(self, mean_dist: np.ndarray, shape: np.ndarray, srp_cutoff: float):
        """Returns (n_red, n_pool, min MI kept)."""
        md = np.ascontiguousarray(mean_dist, dtype=np.float64)
        sh = np.ascontiguousarray(shape, dtype=np.float64)
        assert sh.shape == (md.shape[0], 3)
        nr, npool, mn = C.c_int64(0), C.c_int64(0), C.c_double(0)
        L.check(L.lib().ldw_sr_pvalues(self._ctx, md.shape[0], md.shape[1], L.ptr(md), L.ptr(sh), float(srp_cutoff),
                                       C.byref(nr), C.byref(npool), C.byref(mn)))
        self._n_red, self._n_pool = nr.value, npool.value
        return nr.value, npool.value, mn.value

    def sr_reduced(self):
        n = self._n_red
        row = np.empty(n, dtype=np.int64)
        cc = np.empty(n, dtype=np.int32)
        first = np.empty(n, dtype=np.int32)
        dup = np.empty(n, dtype=np.uint8)
        srp = np.empty(n, dtype=np.float64)
        a = np.empty(n, dtype=np.int32)
        b = np.empty(n, dtype=np.int32)
        mi = np.empty(n, dtype=np.float64)
        L.check(L.lib().ldw_sr_reduced_fetch(self._ctx, n, L.ptr(row), L.ptr(a), L.ptr(b), L.ptr(mi), L.ptr(cc), L.ptr(first),
                                             L.ptr(dup), L.ptr(srp)))
        return dict(row=row, a=a, b=b, MI=mi, clust_c=cc, first_clust=first, dup=dup.astype(bool), srp_max=srp)

    def sr_pool(self):
        n = self._n_pool
        a = np.empty(n, dtype=np.int32)
        b = np.empty(n, dtype=np.int32)
        mi = np.empty(n, dtype=np.float64)
        L.check(L.lib().ldw_sr_pool_fetch(self._ctx, n, L.ptr(a), L.ptr(b), L.ptr(mi)))
        return a, b, mi

    # -- r05: the same model with the table left on the ranks that computed it (dist_srp.py) ---------
    def sr_excess_stats_blocks(self, mean_dist: np.ndarray, rows_per_block) -> np.ndarray:
        """(nblocks, nclust, 5): ldw_sr_excess_stats per reference block of this engine's table (rows of the blocks in order)."""
        md = np.ascontiguousarray(mean_dist, dtype=np.float64)
        rows = np.ascontiguousarray(rows_per_block, dtype=np.int64)
        out = np.zeros((len(rows), md.shape[0], 5), dtype=np.float64)
        L.check(L.lib().ldw_sr_excess_stats_blocks(self._ctx, md.shape[0], md.shape[1], L.ptr(md), len(rows), L.ptr(rows), L.ptr(out)))
        return out

    def sr_tail_extract(self, lower: np.ndarray, on_device: bool = False):
        """Rows at or above ``lower`` (nclust, S) per (cluster, len): (cnt, mi) with cnt (S, nclust) — len-major — and mi their MI values
        grouped in that order: a host array, or (``on_device``) a torch tensor on this engine's GPU — what an RCCL exchange sends as it is."""
        lo = np.ascontiguousarray(lower, dtype=np.float64)
        nclust, S = lo.shape
        cnt = np.zeros((S, nclust), dtype=np.int64)
        n = C.c_int64(0)
        L.check(L.lib().ldw_sr_tail_extract(self._ctx, nclust, S, L.ptr(lo), L.ptr(cnt), None, 0, 0, C.byref(n)))
        if on_device:
            import torch
            dev = torch.device("cuda", self.device)
            mi = torch.empty(n.value, dtype=torch.float64, device=dev)
            if n.value:
                torch.cuda.synchronize(dev)
                L.check(L.lib().ldw_sr_tail_extract(self._ctx, nclust, S, L.ptr(lo), L.ptr(cnt), L.ptr(mi), n.value, 1, C.byref(n)))
            return cnt, mi
        mi = np.empty(n.value, dtype=np.float64)
        if n.value:
            L.check(L.lib().ldw_sr_tail_extract(self._ctx, nclust, S, L.ptr(lo), L.ptr(cnt), L.ptr(mi), n.value, 0, C.byref(n)))
        return cnt, mi

    def sr_quantiles_merge(self, prob: float, cnts: list, mis: list, n_total: np.ndarray):
        """(q_lo, q_hi, violations) of the groups over all ranks from the candidates ``sr_tail_extract`` gave on each (``cnts[r]`` (S, nclust),
        ``mis[r]``) and the groups' global sizes ``n_total`` (nclust, S)."""
        nt = np.ascontiguousarray(n_total, dtype=np.int64)
        nclust, S = nt.shape
        cs = [np.ascontiguousarray(c, dtype=np.int64) for c in cnts]
        assert len(cs) == len(mis) >= 1 and all(c.shape == (S, nclust) for c in cs)
        on_dev = all(_is_torch(m) and m.is_cuda for m in mis)    # (what sr_tail_extract(.., on_device=True) gave and an RCCL gather delivered)
        if on_dev:
            import torch
            ms = [m.contiguous() for m in mis]
            assert all(str(m.dtype) == "torch.float64" and m.device.index == self.device for m in ms)
            torch.cuda.synchronize(ms[0].device)                 # the library reads them on its own stream
            pm = (C.c_void_p * len(ms))(*[m.data_ptr() if m.numel() else None for m in ms])
        else:
            ms = [np.ascontiguousarray(m.cpu().numpy() if _is_torch(m) else m, dtype=np.float64) for m in mis]
            pm = (C.c_void_p * len(ms))(*[m.ctypes.data if m.size else None for m in ms])
        pc = (C.c_void_p * len(cs))(*[c.ctypes.data for c in cs])
        qlo = np.empty((nclust, S), dtype=np.float64)
        qhi = np.empty((nclust, S), dtype=np.float64)
        viol = C.c_int64(0)
        L.check(L.lib().ldw_sr_quantiles_merge(self._ctx, nclust, S, float(prob), len(ms), pm, pc, L.ptr(nt), int(on_dev), L.ptr(qlo), L.ptr(qhi), C.byref(viol)))
        return qlo, qhi, int(viol.value)

    def sr_pvalues_local(self, mean_dist: np.ndarray, shape: np.ndarray, srp_cutoff: float):
        """ldw_sr_pvalues without the pool: (n_red, min MI kept on this engine — NaN when nothing was kept)."""
        md = np.ascontiguousarray(mean_dist, dtype=np.float64)
        sh = np.ascontiguousarray(shape, dtype=np.float64)
        assert sh.shape == (md.shape[0], 3)
        nr, mn = C.c_int64(0), C.c_double(0)
        L.check(L.lib().ldw_sr_pvalues(self._ctx, md.shape[0], md.shape[1], L.ptr(md), L.ptr(sh), float(srp_cutoff), C.byref(nr), None, C.byref(mn)))
        self._n_red, self._n_pool = nr.value, 0
        return nr.value, mn.value

    def sr_pool_build(self, min_mi: float) -> int:
        n = C.c_int64(0)
        L.check(L.lib().ldw_sr_pool_build(self._ctx, float(min_mi), C.byref(n)))
        self._n_pool = n.value
        return n.value

    def sr_reduced_import(self, a, b, mi, pool_a, pool_b, pool_mi):
        """Adopt the kept links and the pool of all ranks; ``aracne_device`` then answers for the kept links in the order given."""
        a, b, mi = L.as_c(a, np.int32), L.as_c(b, np.int32), L.as_c(mi, np.float64)
        pa, pb, pm = L.as_c(pool_a, np.int32), L.as_c(pool_b, np.int32), L.as_c(pool_mi, np.float64)
        assert len(a) == len(b) == len(mi) and len(pa) == len(pb) == len(pm)
        L.check(L.lib().ldw_sr_reduced_import(self._ctx, len(mi), L.ptr(a), L.ptr(b), L.ptr(mi), len(pm), L.ptr(pa), L.ptr(pb), L.ptr(pm)))
        self._n_red, self._n_pool = len(mi), len(pm)

    def aracne_device(self) -> np.ndarray:
        """ARACNE flags of the kept links (order of sr_reduced()) against the device-resident pool."""
        out = np.ones(self._n_red, dtype=np.uint8)
        L.check(L.lib().ldw_aracne_device(self._ctx, self._n_red, L.ptr(out)))
        return out.astype(bool)

    # -- consumers of the link tables ---------------------------
    def lr_tukey(self, min_links: int = 5000, sr=None):
        """Tukey thresholds of the long-range table, outlier links and ARACNE pool left on the device
        (analyse_long_range_links, R/lr_analyser.R:72-111).  ``sr`` = (a, b, MI) of the REDUCED short-range links — the rows of
        sr_links.tsv, which is what the reference pools with the long-range links (R/lr_analyser.R:67,106-109); None: no rows."""
        q13, thr = np.zeros(2), np.zeros(2)
        fb = C.c_int(0)
        nr, npool = C.c_int64(0), C.c_int64(0)
        if sr is None:
            sa = sb = smi = None
            ns = 0
        else:
            sa, sb, smi = L.as_c(sr[0], np.int32), L.as_c(sr[1], np.int32), L.as_c(sr[2], np.float64)
            ns = len(smi)
            assert len(sa) == len(sb) == ns
        L.check(L.lib().ldw_lr_tukey(self._ctx, int(min_links), L.ptr(sa), L.ptr(sb), L.ptr(smi), ns, L.ptr(q13), L.ptr(thr),
                                     C.byref(fb), C.byref(nr), C.byref(npool)))
        self._n_red, self._n_pool = nr.value, npool.value
        return dict(q13=q13, thresholds=thr, fallback=bool(fb.value), n_red=nr.value, n_pool=npool.value)

    def lr_reduced(self):
        n = self._n_red
        row = np.empty(n, dtype=np.int64)
        a = np.empty(n, dtype=np.int32)
        b = np.empty(n, dtype=np.int32)
        mi = np.empty(n, dtype=np.float64)
        L.check(L.lib().ldw_lr_reduced_fetch(self._ctx, n, L.ptr(row), L.ptr(a), L.ptr(b), L.ptr(mi)))
        return dict(row=row, a=a, b=b, MI=mi)

    def ldmap(self, reducer: int = 0, from_: int = 0, to: int = 0, plot_save_path=None, plot_title=None):
        """Block-summed, log-scaled, 0..1-rescaled LD map of all links (genomewide_LDMap, R/LDSummaryPlot.R:55-106).
        Returns (htm [B, B], n_pos, reducer).  ``plot_save_path``: LD_plot.png is written there from the map's device copy (ldw_plot_ldmap)."""
        n_pos, r, B = C.c_int64(0), C.c_int32(0), C.c_int32(0)
        L.check(L.lib().ldw_ldmap(self._ctx, int(reducer), int(from_), int(to), C.byref(n_pos), C.byref(r), C.byref(B), None, 0))
        htm = np.empty((B.value, B.value), dtype=np.float64)
        if plot_save_path is None:
            L.check(L.lib().ldw_ldmap(self._ctx, int(reducer), int(from_), int(to), C.byref(n_pos), C.byref(r), C.byref(B), L.ptr(htm), htm.size))
        else:
            L.check(L.lib().ldw_plot_ldmap(self._ctx, int(reducer), int(from_), int(to), None if plot_title is None else str(plot_title).encode(),
                                           os.fsencode(plot_save_path), C.byref(n_pos), C.byref(r), C.byref(B), L.ptr(htm), htm.size))
        return htm, n_pos.value, r.value

    # -- element-wise twins ------------------------------------------------------
    def acgtn2num(self, nv: np.ndarray, ref_chars) -> None:
        """In-place twin of .ACGTN2num: nv is a Fortran-ordered (5, L) float64 matrix."""
        assert nv.dtype == np.float64 and nv.shape[0] == 5 and nv.flags.f_contiguous
        if isinstance(ref_chars, (bytes, bytearray)):
            ref = bytes(ref_chars)
        else:  # like as<char>(cv[c]): first character of each string ("" -> NUL, leaves the column untouched)
            ref = b"".join((bytes(s[:1]) if isinstance(s, (bytes, bytearray)) else str(s)[:1].encode("latin1")) or b"\0"
                           for s in ref_chars)
        assert len(ref) == nv.shape[1]
        buf = C.create_string_buffer(ref, len(ref))
        L.check(L.lib().ldw_acgtn2num(self._ctx, L.ptr(nv), C.cast(buf, C.c_void_p), nv.shape[1], 1))

    def fast_hadamard(self, MI, den, uq, pxy, pxpy, RXY, pXrX, pYrY) -> None:
        ops = [np.asarray(a, dtype=np.float64).reshape(-1, order="F") for a in (den, uq, pxy, pxpy, RXY, pXrX, pYrY)]
        flat = np.ascontiguousarray(MI.reshape(-1, order="F"))
        L.check(L.lib().ldw_fast_hadamard(self._ctx, L.ptr(flat), *[L.ptr(o) for o in ops], flat.size, 0))
        np.copyto(MI, flat.reshape(MI.shape, order="F"))


def aracne(chk_pos1, chk_pos2, chk_MI, full_pos1, full_pos2, full_MI) -> np.ndarray:
    c = [L.as_c(x, np.float64) for x in (chk_pos1, chk_pos2, chk_MI)]
    f = [L.as_c(x, np.float64) for x in (full_pos1, full_pos2, full_MI)]
    out = np.ones(len(c[0]), dtype=np.uint8)
    L.check(L.lib().ldw_aracne(None, L.ptr(c[0]), L.ptr(c[1]), L.ptr(c[2]), len(c[0]), L.ptr(f[0]), L.ptr(f[1]), L.ptr(f[2]),
                               len(f[0]), L.ptr(out)))
    return out.astype(bool)


def format_number(x: float) -> str:
    """One double as write.table prints it (native twin of rcompat.format_number)."""
    buf = C.create_string_buffer(64)
    L.check(L.lib().ldw_format_number(float(x), buf, 64))
    return buf.value.decode()


def kmeans_1d(x, k: int):
    """k-means of the values x into k clusters at the exact optimum of the within-cluster sum of squares (ldw_kmeans_1d, host only):
    (labels int32 [n] in 1..k by cluster size, descending, cutoff = max(x[labels == 1])).  ValueError as R's kmeans for fewer than k
    distinct values."""
    xs = L.as_c(x, np.float64).ravel()
    lab = np.empty(len(xs), dtype=np.int32)
    cut = C.c_double(0)
    rc = L.lib().ldw_kmeans_1d(L.ptr(xs), len(xs), int(k), L.ptr(lab), C.byref(cut))
    if rc == L.LDW_ERR_ARG:
        raise ValueError(L.lib().ldw_last_error().decode("utf-8", "replace"))
    L.check(rc)
    return lab, float(cut.value)


def write_table_tsv(path: str, columns, append: bool = True, nthreads: int = 0) -> int:
    """write.table(append = T, quote = F, row.names = F, col.names = F, sep = '\\t') of numeric columns by the native
    writer (R/computePairwiseMI.R:140,362): integer arrays print as integers, floating ones by R's 15-digit rule."""
    cols, kinds = [], []
    for c in columns:
        c = np.asarray(c)
        if c.dtype.kind in "iub":
            c = np.ascontiguousarray(c, dtype=np.int64)
            kinds.append(L.COL_INT64)
        else:
            c = np.ascontiguousarray(c, dtype=np.float64)
            kinds.append(L.COL_DOUBLE)
        cols.append(c)
    n = len(cols[0]) if cols else 0
    assert all(len(c) == n for c in cols)
    kind = np.asarray(kinds, dtype=np.int32)
    ptrs = (C.c_void_p * len(cols))(*[c.ctypes.data for c in cols])
    nb = C.c_int64(0)
    L.check(L.lib().ldw_write_table_tsv(str(path).encode(), int(bool(append)), n, len(cols), L.ptr(kind), C.cast(ptrs, C.c_void_p), int(nthreads),
                                        C.byref(nb)))
    return int(nb.value)



class EngineGroup:
    """The short-range model's view of SEVERAL engines of this process after ``Engine.mi_all_pairs_multi(.., sr_rows_stay=True)``: the reductions
    of ``srp.merge_n_sort_sr_links_device`` run over the engines' own rows inside the library (ldw_sr_len_quantiles_multi / _excess_stats_multi /
    _pvalues_multi: a worker thread per context; docs/HISTORY.md 7b), everything after them on engines[0]."""

    def __init__(self, engines):
        self.engines = list(engines)
        self._arr = (C.c_void_p * len(self.engines))(*[e._ctx.value for e in self.engines])
        self.device = self.engines[0].device

    def links_count(self, which: int) -> int:
        return self.engines[0].links_count(which) if which else sum(e.links_count(0) for e in self.engines)

    def sr_len_quantiles(self, nclust: int, sr_dist: float, prob: float = 0.95):
        S = int(np.ceil(sr_dist)) - 1
        qlo = np.empty((nclust, S), dtype=np.float64)
        qhi = np.empty((nclust, S), dtype=np.float64)
        n = np.empty((nclust, S), dtype=np.int64)
        L.check(L.lib().ldw_sr_len_quantiles_multi(self._arr, len(self.engines), int(nclust), float(sr_dist), float(prob), S, L.ptr(qlo), L.ptr(qhi), L.ptr(n)))
        return qlo, qhi, n

    def sr_excess_stats(self, mean_dist: np.ndarray) -> np.ndarray:
        md = np.ascontiguousarray(mean_dist, dtype=np.float64)
        out = np.empty((md.shape[0], 5), dtype=np.float64)
        L.check(L.lib().ldw_sr_excess_stats_multi(self._arr, len(self.engines), md.shape[0], md.shape[1], L.ptr(md), L.ptr(out)))
        return out

    def sr_pvalues(self, mean_dist: np.ndarray, shape: np.ndarray, srp_cutoff: float):
        md = np.ascontiguousarray(mean_dist, dtype=np.float64)
        sh = np.ascontiguousarray(shape, dtype=np.float64)
        assert sh.shape == (md.shape[0], 3)
        nr, npool, mn = C.c_int64(0), C.c_int64(0), C.c_double(0)
        L.check(L.lib().ldw_sr_pvalues_multi(self._arr, len(self.engines), md.shape[0], md.shape[1], L.ptr(md), L.ptr(sh), float(srp_cutoff),
                                             C.byref(nr), C.byref(npool), C.byref(mn)))
        self.engines[0]._n_red, self.engines[0]._n_pool = nr.value, npool.value
        return nr.value, npool.value, mn.value

    def sr_reduced(self):
        return self.engines[0].sr_reduced()

    def sr_pool(self):
        return self.engines[0].sr_pool()

    def aracne_device(self):
        return self.engines[0].aracne_device()
