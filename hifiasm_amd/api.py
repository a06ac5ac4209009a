"""Host-side mirror of the reference seam over the C ABI of libhao.so (include/hao.h).

The reference's interface for this path is three functions:
``ha_ft_gen`` (htab.cpp:1136), ``ha_pt_gen`` (htab.cpp:1232) and ``h_ec_lchain``
(anchor.cpp:2302) plus the accessors ``ha_ft_cnt`` / ``ha_pt_get`` and the finer
``mz1_ha_sketch``.  :class:`Engine` exposes them with the same names, argument
meaning and (absence of) error returns: failures raise :class:`HaoError`, mirroring
the reference's ``exit(1)``.  This module is plumbing only (ctypes + numpy); all
compute happens in the HIP kernels.  There is no CPU fallback: constructing an
Engine without a HIP device raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


SORTDBG_SEQ, SORTDBG_WAVE_LDS, SORTDBG_WAVE_GLOBAL, SORTDBG_BLOCK, SORTDBG_SELECT = range(5)      # hao_dbg_sort_perm's paths (include/hao.h)


class HaoError(RuntimeError):
    pass


class Opt(C.Structure):
    _fields_ = [("k", C.c_int32), ("w", C.c_int32), ("hpc", C.c_int32), ("sample_dist", C.c_int32), ("rewin", C.c_int32),
                ("min_hist_cnt", C.c_int32), ("max_kmer_cnt", C.c_int32), ("max_n_chain", C.c_int32),
                ("high_factor", C.c_double), ("is_ont", C.c_int32), ("bf_shift", C.c_int32), ("hg_size", C.c_int64)]


class Pass(C.Structure):
    """hao_pass_t: the per-pass arguments of h_ec_lchain (anchor.cpp:2302)"""
    _fields_ = [("bw_thres", C.c_double), ("max_n_chain", C.c_int32), ("high_occ", C.c_uint32), ("low_occ", C.c_uint32),
                ("apend_be", C.c_int32), ("is_accurate", C.c_int32), ("gen_off", C.c_int32), ("mcopy_num", C.c_int32),
                ("mcopy_rate", C.c_double), ("chain_cutoff", C.c_uint32), ("mcopy_khit_cut", C.c_uint32), ("ocv_w", C.c_uint64)]


class ChainHdr(C.Structure):
    _fields_ = [("n_hits", C.c_uint32), ("w0", C.c_uint32), ("q0", C.c_uint32), ("offset", C.c_uint32), ("pos", C.c_uint64)]


class Delivery(C.Structure):
    """hao_delivery_t: read-only view of one batch's results in a pinned host arena"""
    _fields_ = [("rid_lo", C.c_uint64), ("n_reads", C.c_uint64), ("n_ol", C.c_uint64), ("n_fc", C.c_uint64), ("n_chains", C.c_uint64),
                ("n_cl", C.c_uint64), ("n_exc", C.c_uint64), ("n_codes", C.c_uint64), ("n_pos", C.c_uint64), ("bytes", C.c_uint64),
                ("ol_off", C.c_void_p), ("ol", C.c_void_p), ("fc_off", C.c_void_p), ("fc", C.c_void_p), ("ch_off", C.c_void_p),
                ("cl_off", C.c_void_p), ("qm_off", C.c_void_p), ("chains", C.c_void_p), ("cl_bits", C.c_void_p), ("cl_rank", C.c_void_p), ("cl_codes", C.c_void_p), ("qmz", C.c_void_p),
                ("cl_exc", C.c_void_p), ("exact", C.c_void_p), ("copy_ms", C.c_double), ("qmz_pos", C.c_void_p), ("qmz_cnt", C.c_void_p)]


class EdDelivery(C.Structure):
    """hao_ed_delivery_t: the window-alignment results of a batch delivered with HAO_DELIVER_ED (pointers into the same pinned arena as its Delivery)"""
    _fields_ = [("n_pairs", C.c_uint64), ("window", C.c_uint32), ("thre", C.c_uint32), ("ed_off", C.c_void_p), ("err", C.c_void_p), ("pe", C.c_void_p),
                ("placement", C.c_uint32), ("pad", C.c_uint32), ("e_rate", C.c_double), ("unresolved", C.c_uint64), ("ovlp", C.c_void_p)]


class TraceDelivery(C.Structure):
    """hao_trace_delivery_t: the traceback of a batch's aligned grid pairs delivered with HAO_DELIVER_TRACE (pointers into the same pinned arena as its Delivery)"""
    _fields_ = [("n_traced", C.c_uint64), ("n_cigar", C.c_uint64), ("cg_off", C.c_void_p), ("ps", C.c_void_p), ("n_cig", C.c_void_p), ("cigar", C.c_void_p)]


class RescueDelivery(C.Structure):
    """hao_rescue_delivery_t: the rescue stage's results of a batch delivered with HAO_DELIVER_RESCUE (pointers into the same pinned arena as its Delivery)"""
    _fields_ = [("n_ol", C.c_uint64), ("n_wins", C.c_uint64), ("n_rescued", C.c_uint64), ("ovlp", C.c_void_p), ("win_off", C.c_void_p), ("wins", C.c_void_p)]


class WlistDelivery(C.Structure):
    """hao_wlist_delivery_t: the window lists of a batch delivered with HAO_DELIVER_WLIST (pointers into the same pinned arena as its Delivery)"""
    _fields_ = [("n_ol", C.c_uint64), ("n_wins", C.c_uint64), ("n_cigar", C.c_uint64), ("n_swept", C.c_uint64), ("n_replace", C.c_uint64), ("n_untraced", C.c_uint64),
                ("win_off", C.c_void_p), ("wins", C.c_void_p), ("cig_off", C.c_void_p), ("cigars", C.c_void_p)]


DELIVER_OL, DELIVER_CL, DELIVER_EXACT, DELIVER_ED, DELIVER_TRACE, DELIVER_RESCUE, DELIVER_WLIST = 1, 2, 4, 8, 16, 32, 64
PLACE_DIAG, PLACE_REF = 0, 1      # hao_ed_delivery_t::placement

ABI_SYMBOLS = [
    "hao_opt_default", "hao_create", "hao_destroy", "hao_last_error", "hao_set_reads", "hao_ft_gen", "hao_pt_gen",
    "hao_ft_cnt", "hao_pt_get", "hao_ft_table", "hao_pt_table", "hao_hist", "hao_stats", "hao_sketch_batch",
    "hao_fetch_sketch", "hao_overlap_batch", "hao_fetch_seed_hits", "hao_fetch_overlaps", "hao_batch_totals", "hao_batch_seed_path", "hao_batch_chain_path",
    "hao_stage_times", "hao_pass_default", "hao_overlap_batch_ex", "hao_set_shard", "hao_dist_unique_id", "hao_dist_init",
    "hao_loop_create", "hao_loop_destroy", "hao_dist_init_loopback", "hao_batch_digest", "hao_selftest_rocprim", "hao_selftest_big", "hao_selftest_sortbits", "hao_unpack_cigar", "hao_unpack_overlaps", "hao_overlap_batch_async", "hao_deliver_wait", "hao_unpack_hits", "hao_exact_check", "hao_fetch_exact", "hao_window_ed_batch", "hao_index_save", "hao_index_load", "hao_next_slot", "hao_attach", "hao_window_trace_batch", "hao_window_ed_long", "hao_window_trace_long", "hao_delivery_digest", "hao_ft_passes", "hao_ovlp_bin_read", "hao_ovlp_bin_write", "hao_window_ed_grid", "hao_fetch_ed_grid",
    "hao_deliver_ed_config", "hao_deliver_ed", "hao_unpack_ed",
    "hao_window_trace_grid", "hao_fetch_trace_grid", "hao_deliver_trace", "hao_unpack_trace",
    "hao_window_ed_ref", "hao_fetch_ed_ovlp", "hao_deliver_ed_config_ref", "hao_ref_thresholds",
    "hao_window_rescue_ref", "hao_fetch_rescue", "hao_rescue_task", "hao_deliver_rescue", "hao_unpack_rescue",
    "hao_window_wlist_ref", "hao_fetch_wlist", "hao_deliver_wlist", "hao_unpack_wlist",
    "hao_dist_gather_reads", "hao_reads_digest", "hao_index_load_dist", "hao_shard_layout",
    "hao_window_ladder", "hao_fetch_ladder", "hao_ladder_thresholds",
    "hao_window_ladder_adv", "hao_fetch_ladder_adv", "hao_ladder_adv_thresholds",
    "hao_window_estimate_err", "hao_fetch_ladder_adv_estimates", "hao_estimate_err_records",
]


RESCUE_OVLP = np.dtype([("verdict", np.uint16), ("flags", np.uint16), ("exit_win", np.uint32), ("align_length", np.uint32), ("n_rescued", np.uint32)])
RESCUE_FWD, RESCUE_BWD, RESCUE_ANCHOR, RESCUE_UNTRACED, RESCUE_NO_EXIT = 0, 1, 2, 1, 0xFFFFFFFF
# hao_ladder_req_t / hao_ladder_res_t (hao_window_ladder) and the result's flags
LADDER_REQ = np.dtype([("ol", np.uint32), ("mode", np.uint32), ("qs", np.int32), ("qe", np.int32), ("ts", np.int32), ("te", np.int32), ("estimate_err", np.int32), ("reserved", np.uint32)])
LADDER_RES = np.dtype([("rung", np.uint32), ("thre", np.int32), ("qs", np.int32), ("qe", np.int32), ("ts", np.int32), ("te", np.int32), ("aux_beg", np.int32), ("flags", np.uint32),
                       ("err", np.int32), ("a_ps", np.int32), ("a_pe", np.int32), ("a_ts", np.int32), ("a_te", np.int32), ("n_cigar", np.int32)])
LADDER_REFUSED, LADDER_UNTRACED = 1, 2
# hao_ladder_adv_res_t (hao_window_ladder_adv), its further flag and the rung id of the exact shortcut
LADDER_ADV_RES = np.dtype([("done", np.int32)] + [(n, LADDER_RES.fields[n][0]) for n in LADDER_RES.names])
LADDER_REPEAT, LADDER_RUNG_EXACT = 4, 6
WLIST_PRIMARY, WLIST_UNTRACED = 3, 1 << 19      # hao_wlist_win_t::info: source of a first-placement window the rescue did not trace; the untraced flag


def wlist_records(raw):
    """hao_wlist_win_t records (uint32 [m, 4]) -> int64 [m, 8]: grid window, y_start, y_end, err, thre, source, re-placed, untraced"""
    raw = np.asarray(raw, dtype=np.uint32).reshape(-1, 4)
    out = np.zeros((raw.shape[0], 8), dtype=np.int64)
    out[:, :7] = rescue_records(raw)
    out[:, 7] = (raw[:, 3].astype(np.int64) >> 19) & 1
    return out


def rescue_records(raw):
    """hao_rescue_win_t records (uint32 [m, 4]) -> int64 [m, 7]: grid window, y_start, y_end, err, thre, direction, re-placed"""
    raw = np.asarray(raw, dtype=np.uint32).reshape(-1, 4)
    out = np.zeros((raw.shape[0], 7), dtype=np.int64)
    out[:, 0] = raw[:, 2]; out[:, 1] = raw[:, 0].view(np.int32) if raw.shape[0] else 0; out[:, 2] = raw[:, 1].view(np.int32) if raw.shape[0] else 0
    info = raw[:, 3].astype(np.int64)
    out[:, 3] = info & 0xFF; out[:, 4] = (info >> 8) & 0xFF; out[:, 5] = (info >> 16) & 3; out[:, 6] = (info >> 18) & 1
    return out


def unpack_rescue(d, e, r, lengths, rid):
    """hao_unpack_rescue (host code) over the three views -> (ovlp structured array, list of int64 [m, 7] record arrays per overlap)"""
    L = np.ascontiguousarray(lengths, dtype=np.uint32)
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    f = lib().hao_unpack_rescue
    n = int(f(C.byref(d), C.byref(e), C.byref(r), L.ctypes.data_as(u32p), rid, None, None, None, 0, 0))
    if n == 2**64 - 1:
        raise HaoError(f"hao_unpack_rescue: read {rid}: the views do not belong together")
    ov = np.zeros(n, dtype=RESCUE_OVLP); wo = np.zeros(n + 1, dtype=np.uint64)
    m = 0
    if n:
        oo = _arr(d.ol_off + 8 * (rid - d.rid_lo), 2, np.uint64)
        ww = _arr(r.win_off + 8 * int(oo[0]), n + 1, np.uint64)
        m = int(ww[n] - ww[0])
    raw = np.zeros((max(m, 1), 4), dtype=np.uint32)
    got = int(f(C.byref(d), C.byref(e), C.byref(r), L.ctypes.data_as(u32p), rid, ov.ctypes.data_as(C.c_void_p), wo.ctypes.data_as(u64p), raw.ctypes.data_as(C.c_void_p), n, m))
    if got != n:
        raise HaoError(f"hao_unpack_rescue: read {rid}: {got} != {n}")
    return ov, [rescue_records(raw[int(wo[i]):int(wo[i + 1])]) for i in range(n)]


def _wlist_split(wo, raw, co, cig):
    recs = wlist_records(raw)
    return [(recs[int(wo[i]):int(wo[i + 1])], [cig[int(co[j]):int(co[j + 1])].copy() for j in range(int(wo[i]), int(wo[i + 1]))]) for i in range(len(wo) - 1)]


def unpack_wlist(d, e, r, w, lengths, rid):
    """hao_unpack_wlist (host code) over the four views -> fetch_wlist's shapes: one (wins int64 [m, 8], [uint16 cigar per record]) per overlap of read rid"""
    L = np.ascontiguousarray(lengths, dtype=np.uint32)
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    f = lib().hao_unpack_wlist
    args = (C.byref(d), C.byref(e), C.byref(r), C.byref(w), L.ctypes.data_as(u32p), rid)
    n = int(f(*args, None, None, None, None, 0, 0, 0))
    if n == 2**64 - 1:
        raise HaoError(f"hao_unpack_wlist: read {rid}: the views do not belong together")
    m = k = 0
    if n:
        oo = _arr(d.ol_off + 8 * (rid - d.rid_lo), 2, np.uint64)
        ww = _arr(w.win_off + 8 * int(oo[0]), n + 1, np.uint64)
        m = int(ww[n] - ww[0])
        if m:
            cc = _arr(w.cig_off + 8 * int(ww[0]), m + 1, np.uint64)
            k = int(cc[m] - cc[0])
    wo = np.zeros(n + 1, dtype=np.uint64); raw = np.zeros((max(m, 1), 4), dtype=np.uint32); co = np.zeros(m + 1, dtype=np.uint64); cig = np.zeros(max(k, 1), dtype=np.uint16)
    got = int(f(*args, wo.ctypes.data_as(u64p), raw.ctypes.data_as(C.c_void_p), co.ctypes.data_as(u64p), cig.ctypes.data_as(C.c_void_p), n, m, k))
    if got != n:
        raise HaoError(f"hao_unpack_wlist: read {rid}: {got} != {n}")
    return _wlist_split(wo, raw[:m], co, cig[:k])


def rescue_task(z, win, window, toff, tab, target_len):
    """hao_rescue_task (host code): the task (uint32 [10]) of the rescue alignment of grid window `win` of overlap z (uint32 [12]) from target offset toff, or None"""
    z = np.ascontiguousarray(z, dtype=np.uint32); tab = np.ascontiguousarray(tab, dtype=np.uint8); out = np.zeros(10, dtype=np.uint32)
    ok = lib().hao_rescue_task(z.ctypes.data_as(C.c_void_p), C.c_uint32(int(win)), C.c_uint32(int(window)), C.c_int64(int(toff)), tab.ctypes.data_as(C.POINTER(C.c_uint8)),
                               C.c_uint32(int(target_len)), out.ctypes.data_as(C.c_void_p))
    return out if ok else None


def lib_path():
    return os.path.join(_HERE, "libhao.so")


def lib():
    global _LIB
    if _LIB is None:
        p = lib_path()
        if not os.path.exists(p):
            raise HaoError(f"{p} is missing - build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(p)
        vp, u8p, u32p, u64p, i64p = C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_int64)
        L.hao_opt_default.argtypes = [C.POINTER(Opt)]
        L.hao_create.argtypes = [C.c_int, C.POINTER(Opt), C.POINTER(vp)]
        L.hao_destroy.argtypes = [vp]
        L.hao_attach.argtypes = [vp, C.POINTER(vp)]
        L.hao_last_error.argtypes = [vp]; L.hao_last_error.restype = C.c_char_p
        L.hao_set_reads.argtypes = [vp, u8p, u64p, u32p, C.c_uint64, u64p, u32p]
        L.hao_ft_gen.argtypes = [vp, C.POINTER(C.c_int32)]
        L.hao_pt_gen.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.hao_ft_cnt.argtypes = [vp, C.c_uint64]; L.hao_ft_cnt.restype = C.c_int32
        L.hao_pt_get.argtypes = [vp, C.c_uint64, C.POINTER(u64p), C.POINTER(C.c_int32)]
        L.hao_ft_table.argtypes = [vp, u64p, C.POINTER(u64p), C.POINTER(C.POINTER(C.c_int32))]
        L.hao_pt_table.argtypes = [vp, u64p, C.POINTER(u64p), C.POINTER(u64p), C.POINTER(u64p), u64p]
        L.hao_hist.argtypes = [vp, C.c_int, i64p]
        L.hao_stats.argtypes = [vp, i64p]
        L.hao_ft_passes.argtypes = [vp]; L.hao_ft_passes.restype = C.c_int
        L.hao_sketch_batch.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_int, C.c_int]
        L.hao_fetch_sketch.argtypes = [vp, C.c_uint64, C.POINTER(vp), u64p]
        L.hao_overlap_batch.argtypes = [vp, C.c_uint64, C.c_uint64]
        L.hao_pass_default.argtypes = [vp, C.POINTER(Pass)]
        L.hao_overlap_batch_ex.argtypes = [vp, C.c_uint64, C.c_uint64, C.POINTER(Pass)]
        L.hao_fetch_seed_hits.argtypes = [vp, C.c_uint64, C.POINTER(vp), u64p]
        L.hao_fetch_overlaps.argtypes = [vp, C.c_uint64, C.POINTER(vp), u64p, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), u64p]
        L.hao_batch_totals.argtypes = [vp, u64p]
        L.hao_batch_seed_path.argtypes = [vp, u64p]
        L.hao_batch_chain_path.argtypes = [vp, u64p]
        L.hao_stage_times.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.c_int]
        L.hao_batch_digest.argtypes = [vp, u64p, u64p]
        L.hao_overlap_batch_async.argtypes = [vp, C.c_uint64, C.c_uint64, C.POINTER(Pass), C.c_uint32, C.POINTER(C.c_int)]
        L.hao_deliver_wait.argtypes = [vp, C.c_int, C.POINTER(Delivery)]
        L.hao_exact_check.argtypes = [vp]
        L.hao_window_ed_batch.argtypes = [vp, vp, C.c_uint64, vp]
        L.hao_window_trace_batch.argtypes = [vp, C.c_int, vp, C.c_uint64, vp, vp, C.c_uint32]
        L.hao_window_ed_long.argtypes = [vp, vp, C.c_uint64, vp]
        L.hao_window_trace_long.argtypes = [vp, C.c_int, vp, C.c_uint64, vp, vp, C.c_uint32]
        L.hao_window_ladder.argtypes = [vp, vp, C.c_uint64, C.c_double, C.c_int64, C.c_int64, vp, vp, vp, C.c_uint64, u64p]
        L.hao_fetch_ladder.argtypes = [vp, vp, C.c_uint64, u64p, u64p]
        L.hao_ladder_thresholds.argtypes = [C.c_int64, C.c_int64, C.c_double, C.c_int64, C.c_int64, C.POINTER(C.c_int32)]
        L.hao_window_ladder_adv.argtypes = [vp, vp, C.c_uint64, C.c_double, C.c_int64, C.c_int64, C.c_int64, C.c_int64, vp, vp, vp, C.c_uint64, u64p]
        L.hao_fetch_ladder_adv.argtypes = [vp, vp, C.c_uint64, u64p, u64p]
        L.hao_ladder_adv_thresholds.argtypes = [C.c_int64, C.c_int64, C.c_double, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.hao_window_estimate_err.argtypes = [vp, vp, C.c_uint64, C.c_double, C.c_int64, vp]
        L.hao_fetch_ladder_adv_estimates.argtypes = [vp, vp, C.c_uint64]
        L.hao_fetch_ladder_adv_estimates.restype = C.c_uint64
        L.hao_estimate_err_records.argtypes = [vp, vp, C.c_uint64, C.c_int64, C.c_int64, C.c_int64, C.c_double]
        L.hao_estimate_err_records.restype = C.c_int64
        L.hao_index_save.argtypes = [vp, C.c_char_p, C.c_int32, vp]
        L.hao_index_load.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int32)]
        L.hao_index_load_dist.argtypes = [vp, C.c_char_p, u64p, C.POINTER(C.c_int32)]
        L.hao_shard_layout.argtypes = [vp, u64p, u64p, u64p, C.POINTER(u32p)]
        L.hao_fetch_exact.argtypes = [vp, C.c_uint64, C.POINTER(vp), u64p]
        L.hao_unpack_hits.argtypes = [C.POINTER(Delivery), C.c_uint64, vp, C.c_uint64]; L.hao_unpack_hits.restype = C.c_uint64
        L.hao_unpack_cigar.argtypes = [C.POINTER(Delivery), C.c_uint64, vp, C.c_uint32]; L.hao_unpack_cigar.restype = C.c_uint32
        L.hao_unpack_overlaps.argtypes = [C.POINTER(Delivery), C.c_uint64, vp, C.c_uint64]; L.hao_unpack_overlaps.restype = C.c_uint64
        L.hao_delivery_digest.argtypes = [C.POINTER(Delivery), u64p, C.c_int]
        L.hao_deliver_ed_config.argtypes = [vp, C.c_uint32, C.c_uint32]
        L.hao_deliver_ed.argtypes = [vp, C.c_int, C.POINTER(EdDelivery)]
        L.hao_unpack_ed.argtypes = [C.POINTER(EdDelivery), C.POINTER(Delivery), u32p, C.c_uint64, vp, vp, C.c_uint64]; L.hao_unpack_ed.restype = C.c_uint64
        L.hao_window_trace_grid.argtypes = [vp, C.c_uint32, C.c_uint32, u64p]
        L.hao_window_ed_ref.argtypes = [vp, C.c_uint32, C.c_double, u64p, u64p]
        L.hao_fetch_ed_ovlp.argtypes = [vp, C.c_uint64, C.POINTER(vp), u64p]
        L.hao_deliver_ed_config_ref.argtypes = [vp, C.c_uint32, C.c_double]
        L.hao_window_rescue_ref.argtypes = [vp, u64p]
        L.hao_deliver_rescue.argtypes = [vp, C.c_int, C.POINTER(RescueDelivery)]
        L.hao_unpack_rescue.argtypes = [C.POINTER(Delivery), C.POINTER(EdDelivery), C.POINTER(RescueDelivery), u32p, C.c_uint64, vp, u64p, vp, C.c_uint64, C.c_uint64]
        L.hao_unpack_rescue.restype = C.c_uint64
        L.hao_fetch_rescue.argtypes = [vp, C.c_uint64, C.POINTER(vp), u64p, C.POINTER(vp), C.POINTER(vp)]
        L.hao_rescue_task.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_int64, u8p, C.c_uint32, vp]
        L.hao_window_wlist_ref.argtypes = [vp, u64p]
        L.hao_deliver_wlist.argtypes = [vp, C.c_int, C.POINTER(WlistDelivery)]
        L.hao_unpack_wlist.argtypes = [C.POINTER(Delivery), C.POINTER(EdDelivery), C.POINTER(RescueDelivery), C.POINTER(WlistDelivery), u32p, C.c_uint64, u64p, vp, u64p, vp, C.c_uint64, C.c_uint64, C.c_uint64]
        L.hao_unpack_wlist.restype = C.c_uint64
        L.hao_fetch_wlist.argtypes = [vp, C.c_uint64, u64p, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
        L.hao_ref_thresholds.argtypes = [C.c_uint32, C.c_double, u8p]; L.hao_ref_thresholds.restype = None
        L.hao_fetch_trace_grid.argtypes = [vp, vp, vp, u64p, vp, C.c_uint64, C.c_uint64]
        L.hao_deliver_trace.argtypes = [vp, C.c_int, C.POINTER(TraceDelivery)]
        L.hao_unpack_trace.argtypes = [C.POINTER(TraceDelivery), C.POINTER(EdDelivery), C.POINTER(Delivery), u32p, C.c_uint64, vp, vp, u64p, vp, C.c_uint64, C.c_uint64]
        L.hao_unpack_trace.restype = C.c_uint64
        L.hao_set_shard.argtypes = [vp, C.c_uint64, C.c_uint64, u32p]
        L.hao_dist_unique_id.argtypes = [u8p]
        L.hao_dist_init.argtypes = [vp, u8p, C.c_int, C.c_int]
        L.hao_loop_create.argtypes = [C.c_int]; L.hao_loop_create.restype = vp
        L.hao_loop_destroy.argtypes = [vp]
        L.hao_dist_init_loopback.argtypes = [vp, vp, C.c_int]
        L.hao_dist_gather_reads.argtypes = [vp]
        L.hao_reads_digest.argtypes = [vp, u64p]
        L.hao_dbg_sort_perm.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_uint64, u64p, u64p, C.POINTER(C.c_int32), u32p]
        _LIB = L
    return _LIB


def _arr(ptr, n, dtype):
    if n == 0 or not ptr:
        return np.zeros(0, dtype=dtype)
    nbytes = int(n) * np.dtype(dtype).itemsize
    addr = ptr if isinstance(ptr, int) else C.cast(ptr, C.c_void_p).value
    return np.frombuffer((C.c_uint8 * nbytes).from_address(addr), dtype=dtype).copy()


class Engine:
    """One engine per GPU (one process per GPU).  Options mirror hifiasm_opt_t."""

    def __init__(self, device: int = 0, **opts):
        self.L = lib()
        self.opt = Opt()
        self.L.hao_opt_default(C.byref(self.opt))
        self.bw_thres = opts.pop("bw_thres", None)      # a per-pass argument of h_ec_lchain, not an option: overrides hao_pass_default's value
        for k, v in opts.items():
            if not hasattr(self.opt, k):
                raise HaoError(f"unknown option {k}")
            setattr(self.opt, k, v)
        h = C.c_void_p()
        rc = self.L.hao_create(device, C.byref(self.opt), C.byref(h))
        if rc != 0:
            raise HaoError(f"hao_create failed ({rc}): no usable HIP device - this engine has no CPU fallback")
        self.h = h
        self.n_reads = 0

    def attach(self):
        """hao_attach: a second batch context (own stream, scratch, results) over this engine's reads and index, for a second host thread"""
        v = Engine.__new__(Engine)
        v.L = self.L; v.opt = self.opt; v.bw_thres = self.bw_thres; v.n_reads = self.n_reads; v.owner = self; v.lengths = getattr(self, "lengths", None); v.rid_base = getattr(self, "rid_base", 0)
        h = C.c_void_p()
        self._ck(self.L.hao_attach(self.h, C.byref(h)), "hao_attach")
        v.h = h
        return v

    def close(self):
        if getattr(self, "h", None):
            self.L.hao_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, what):
        if rc != 0:
            raise HaoError(f"{what} failed ({rc}): {self.L.hao_last_error(self.h).decode()}")

    # ---- read store (All_reads, Process_Read.h:115-146) ----
    def set_reads(self, packed, pk_off, lengths, n_mask=None, code_off=None):
        """packed/pk_off/lengths as produced by ha_compress_base; n_mask (per-base 0/1, with code_off) lists N sites."""
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        pk_off = np.ascontiguousarray(pk_off, dtype=np.uint64)
        lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
        n = lengths.size
        ns_off = ns = None
        if n_mask is not None:
            pos = np.flatnonzero(n_mask).astype(np.uint64)
            co = np.ascontiguousarray(code_off, dtype=np.uint64)
            rid = np.searchsorted(co, pos, side="right") - 1
            ns = (pos - co[rid]).astype(np.uint32)
            ns_off = np.zeros(n + 1, dtype=np.uint64)
            np.cumsum(np.bincount(rid, minlength=n), out=ns_off[1:], dtype=np.uint64)
        u8p, u32p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
        self._ck(self.L.hao_set_reads(self.h, packed.ctypes.data_as(u8p), pk_off.ctypes.data_as(u64p), lengths.ctypes.data_as(u32p), n,
                                      ns_off.ctypes.data_as(u64p) if ns_off is not None else None,
                                      ns.ctypes.data_as(u32p) if ns is not None else None), "hao_set_reads")
        self.n_reads = n
        self.lengths = lengths.copy()      # (hao_unpack_ed rebuilds delivered window pairs from the lengths of all reads)

    def set_readset(self, rs):
        self.set_reads(rs.packed, rs.pk_off, rs.lengths, rs.n_mask(), rs.code_off)

    # ---- sharded mode (one process per GPU; reads partitioned by query read) ----
    def set_shard(self, rid_base, all_lengths):
        al = np.ascontiguousarray(all_lengths, dtype=np.uint32)
        self._ck(self.L.hao_set_shard(self.h, int(rid_base), al.size, al.ctypes.data_as(C.POINTER(C.c_uint32))), "hao_set_shard")
        self.rid_base = int(rid_base)

    @staticmethod
    def dist_unique_id():
        buf = (C.c_uint8 * 128)()
        if lib().hao_dist_unique_id(buf) != 0:
            raise HaoError("hao_dist_unique_id failed")
        return bytes(buf)

    def dist_init(self, uid: bytes, rank: int, world: int):
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        self._ck(self.L.hao_dist_init(self.h, buf, rank, world), "hao_dist_init")

    def dist_init_loopback(self, group, rank: int):
        self._ck(self.L.hao_dist_init_loopback(self.h, group, rank), "hao_dist_init_loopback")

    def dist_gather_reads(self):
        """hao_dist_gather_reads (a collective): the bases of ALL reads on every rank of a sharded engine, which opens the exact check and the window-alignment
        stages to it; a no-op on an unsharded engine and while the store is valid"""
        self._ck(self.L.hao_dist_gather_reads(self.h), "hao_dist_gather_reads")

    def reads_digest(self):
        """hao_reads_digest: (bases, N sites) digests of the reads the stages beyond the seam see - equal on every rank of a sharded engine and on an unsharded one"""
        out = (C.c_uint64 * 2)()
        self._ck(self.L.hao_reads_digest(self.h, out), "hao_reads_digest")
        return int(out[0]), int(out[1])

    def dbg_sort_perm(self, mode, path, arrays, variant=0, off=None):
        """hao_dbg_sort_perm: one of the selection's sorts alone (path: SORTDBG_*) on key arrays [(xs, sc)]; mode 0 sorts by sc descending, mode 1 by xs ascending.
        Returns one permutation per array (index within the array of the key at every slot).  off: offsets to pass instead of the arrays' own (tests of the refusals)."""
        xs = np.ascontiguousarray(np.concatenate([np.asarray(a[0], dtype=np.uint64) for a in arrays] + [np.zeros(1, np.uint64)]))
        sc = np.ascontiguousarray(np.concatenate([np.asarray(a[1], dtype=np.int32) for a in arrays] + [np.zeros(1, np.int32)]))
        own = np.concatenate([[0], np.cumsum([len(a[0]) for a in arrays])]).astype(np.uint64)
        o = own if off is None else np.ascontiguousarray(off, dtype=np.uint64)
        perm = np.full(int(own[-1]) + 1, 0xffffffff, dtype=np.uint32)
        self._ck(self.L.hao_dbg_sort_perm(self.h, mode, path, variant, len(o) - 1, *[a.ctypes.data_as(C.POINTER(t)) for a, t in ((o, C.c_uint64), (xs, C.c_uint64), (sc, C.c_int32), (perm, C.c_uint32))]), "hao_dbg_sort_perm")
        return [perm[int(own[i]):int(own[i + 1])].astype(np.int64) for i in range(len(arrays))]

    def delivery_global(self, d):
        """a copy of a sharded engine's Delivery with rid_lo as a GLOBAL read id: what the delivered_* / hao_unpack_* helpers take together with the lengths
        of all reads and global read ids (they index one lengths array by the delivery's read ids and by y_id)"""
        g = Delivery.from_buffer_copy(d)
        g.rid_lo = int(d.rid_lo) + getattr(self, "rid_base", 0)
        for k in ("ed", "tr", "rs", "wl"):
            setattr(g, k, getattr(d, k, None))
        return g

    # ---- ha_ft_gen / ha_pt_gen ----
    def ha_ft_gen(self):
        hom = C.c_int32()
        self._ck(self.L.hao_ft_gen(self.h, C.byref(hom)), "hao_ft_gen")
        return hom.value

    def ha_pt_gen(self):
        hom, het = C.c_int32(), C.c_int32()
        self._ck(self.L.hao_pt_gen(self.h, C.byref(hom), C.byref(het)), "hao_pt_gen")
        return hom.value, het.value

    def ha_ft_cnt(self, y):
        return self.L.hao_ft_cnt(self.h, y)

    def ha_pt_get(self, y):
        p, n = C.POINTER(C.c_uint64)(), C.c_int32()
        self._ck(self.L.hao_pt_get(self.h, y, C.byref(p), C.byref(n)), "hao_pt_get")
        return _arr(p, n.value, np.uint64)

    def ft_table(self):
        n, k, v = C.c_uint64(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_int32)()
        self._ck(self.L.hao_ft_table(self.h, C.byref(n), C.byref(k), C.byref(v)), "hao_ft_table")
        return _arr(k, n.value, np.uint64), _arr(v, n.value, np.int32)

    def pt_table(self):
        nk, npos = C.c_uint64(), C.c_uint64()
        k, o, p = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)()
        self._ck(self.L.hao_pt_table(self.h, C.byref(nk), C.byref(k), C.byref(o), C.byref(p), C.byref(npos)), "hao_pt_table")
        return _arr(k, nk.value, np.uint64), _arr(o, nk.value + 1, np.uint64), _arr(p, npos.value, np.uint64)

    def hist(self, which):
        out = (C.c_int64 * 4096)()
        self._ck(self.L.hao_hist(self.h, which, out), "hao_hist")
        return np.array(out, dtype=np.int64)

    def stats(self):
        out = (C.c_int64 * 8)()
        self._ck(self.L.hao_stats(self.h, out), "hao_stats")
        names = ["ft_peak_hom", "ft_peak_het", "ft_cutoff", "max_n_chain", "hom_cov", "het_cov", "high_occ", "low_occ"]
        return dict(zip(names, [int(x) for x in out]))

    def ft_passes(self):
        """hash-range passes the last ha_ft_gen counted in"""
        return int(self.L.hao_ft_passes(self.h))

    # ---- mz1_ha_sketch ----
    def sketch_batch(self, lo, hi, use_ft=True, sample_dist=None):
        sd = self.opt.sample_dist if sample_dist is None else sample_dist
        self._ck(self.L.hao_sketch_batch(self.h, lo, hi, int(use_ft), sd), "hao_sketch_batch")

    def fetch_sketch(self, rid):
        p, n = C.c_void_p(), C.c_uint64()
        self._ck(self.L.hao_fetch_sketch(self.h, rid, C.byref(p), C.byref(n)), "hao_fetch_sketch")
        return _arr(p.value, 2 * n.value, np.uint64).reshape(-1, 2)

    # ---- h_ec_lchain ----
    def pass_default(self):
        p = Pass()
        self._ck(self.L.hao_pass_default(self.h, C.byref(p)), "hao_pass_default")
        if self.bw_thres is not None:
            p.bw_thres = self.bw_thres
        return p

    def overlap_batch(self, lo, hi, bw_thres=None):
        """h_ec_lchain for reads [lo, hi) with worker_hap_ec's arguments (ecovlp.cpp:3274); bw_thres = 0.001 gives the final-round call (:3957)"""
        if bw_thres is None and self.bw_thres is None:
            self._ck(self.L.hao_overlap_batch(self.h, lo, hi), "hao_overlap_batch")
            return
        p = self.pass_default()
        if bw_thres is not None:
            p.bw_thres = bw_thres
        self._ck(self.L.hao_overlap_batch_ex(self.h, lo, hi, C.byref(p)), "hao_overlap_batch_ex")

    # ---- streaming delivery (hao_overlap_batch_async / hao_deliver_wait / hao_unpack_hits) ----
    def overlap_batch_async(self, lo, hi, parts=DELIVER_OL | DELIVER_CL, bw_thres=None):
        """compute reads [lo, hi) and queue the copy of their results into a pinned host arena; returns the arena slot (0 / 1).  At most two batches are
        in flight: the slot is reused by the second-next async batch."""
        p = None
        if bw_thres is not None or self.bw_thres is not None:
            p = self.pass_default()
            if bw_thres is not None:
                p.bw_thres = bw_thres
        slot = C.c_int(-1)
        self._ck(self.L.hao_overlap_batch_async(self.h, lo, hi, C.byref(p) if p is not None else None, parts, C.byref(slot)), "hao_overlap_batch_async")
        if not hasattr(self, "_ed_slot"):
            self._ed_slot = {}
        self._ed_slot[slot.value] = bool(parts & DELIVER_ED)
        if not hasattr(self, "_tr_slot"):
            self._tr_slot = {}
        self._tr_slot[slot.value] = bool(parts & DELIVER_TRACE)
        if not hasattr(self, "_rs_slot"):
            self._rs_slot = {}
        self._rs_slot[slot.value] = bool(parts & DELIVER_RESCUE)
        if not hasattr(self, "_wl_slot"):
            self._wl_slot = {}
        self._wl_slot[slot.value] = bool(parts & DELIVER_WLIST)
        return slot.value

    def deliver_wait(self, slot):
        """the Delivery view of a slot (blocks until its copy has landed); with DELIVER_ED its window-alignment view rides along as ``d.ed``"""
        d = Delivery()
        self._ck(self.L.hao_deliver_wait(self.h, slot, C.byref(d)), "hao_deliver_wait")
        d.ed = self.deliver_ed(slot) if getattr(self, "_ed_slot", {}).get(slot) else None
        d.tr = self.deliver_trace(slot) if getattr(self, "_tr_slot", {}).get(slot) else None
        d.rs = self.deliver_rescue(slot) if getattr(self, "_rs_slot", {}).get(slot) else None
        d.wl = self.deliver_wlist(slot) if getattr(self, "_wl_slot", {}).get(slot) else None
        return d

    def deliver_ed_config(self, window=375, thre=15):
        """the window grid of this context's DELIVER_ED batches (hao_deliver_ed_config: windows of `window` query bases, threshold thre)"""
        self._ck(self.L.hao_deliver_ed_config(self.h, C.c_uint32(window), C.c_uint32(thre)), "hao_deliver_ed_config")

    def deliver_ed_config_ref(self, window=775, e_rate=0.04):
        """this context's following DELIVER_ED batches in REFERENCE placement (hao_deliver_ed_config_ref): the fake-cigar shift of the window's target start, one
        threshold per window from its length and e_rate, init_waln's admission and clipping; deliver_ed_config switches back"""
        self._ck(self.L.hao_deliver_ed_config_ref(self.h, C.c_uint32(window), C.c_double(e_rate)), "hao_deliver_ed_config_ref")

    def delivered_ed_ovlp(self, d, rid):
        """uint32 [n_ol, 4] (windows covered, windows aligned, aligned bases, error sum) of read rid's overlaps out of a reference-placed DELIVER_ED batch"""
        e = getattr(d, "ed", None)
        if e is None or not e.ovlp:
            raise HaoError("delivered_ed_ovlp: the batch was not delivered with DELIVER_ED in reference placement")
        oo = _arr(d.ol_off + 8 * (rid - d.rid_lo), 2, np.uint64)
        return _arr(e.ovlp + 16 * int(oo[0]), 4 * int(oo[1] - oo[0]), np.uint32).reshape(-1, 4)

    def deliver_ed(self, slot):
        """the EdDelivery view of a waited-for slot whose batch asked for DELIVER_ED"""
        e = EdDelivery()
        self._ck(self.L.hao_deliver_ed(self.h, slot, C.byref(e)), "hao_deliver_ed")
        return e

    def delivered_ed(self, d, rid, lengths=None):
        """(tasks uint32 [n,10], results int32 [n,2]) of read rid's window pairs out of a Delivery with DELIVER_ED - fetch_ed_grid's shapes and values for the read:
        the tasks rebuilt from the delivered overlaps (hao_unpack_ed), the results widened (err INT32_MAX / pe -1 without an alignment)"""
        e = getattr(d, "ed", None)
        if e is None:
            raise HaoError("delivered_ed: the batch was not delivered with DELIVER_ED")
        if lengths is None:
            lengths = getattr(self, "lengths", None)
        if lengths is None:
            raise HaoError("delivered_ed: the lengths of all reads are needed (pass lengths=)")
        L = np.ascontiguousarray(lengths, dtype=np.uint32)
        u32p = C.POINTER(C.c_uint32)
        n = int(self.L.hao_unpack_ed(C.byref(e), C.byref(d), L.ctypes.data_as(u32p), rid, None, None, 0))
        t = np.zeros((n, 10), dtype=np.uint32); r = np.zeros((n, 2), dtype=np.int32)
        got = int(self.L.hao_unpack_ed(C.byref(e), C.byref(d), L.ctypes.data_as(u32p), rid, t.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), n))
        if got != n:
            raise HaoError(f"hao_unpack_ed: read {rid}: the pairs rebuilt from the delivered overlaps do not match the delivered count (lengths of another read set?)")
        return t, r

    def deliver_rescue(self, slot):
        """the RescueDelivery view of a waited-for slot whose batch asked for DELIVER_RESCUE"""
        r = RescueDelivery()
        self._ck(self.L.hao_deliver_rescue(self.h, slot, C.byref(r)), "hao_deliver_rescue")
        return r

    def delivered_rescue(self, d, rid, lengths=None):
        """(ovlp, wins) of read rid out of a Delivery with DELIVER_ED | DELIVER_RESCUE - fetch_rescue's shapes and values (hao_unpack_rescue)"""
        r, e = getattr(d, "rs", None), getattr(d, "ed", None)
        if r is None or e is None:
            raise HaoError("delivered_rescue: the batch was not delivered with DELIVER_ED | DELIVER_RESCUE")
        if lengths is None:
            lengths = getattr(self, "lengths", None)
        if lengths is None:
            raise HaoError("delivered_rescue: the lengths of all reads are needed (pass lengths=)")
        return unpack_rescue(d, e, r, lengths, rid)

    def deliver_trace(self, slot):
        """the TraceDelivery view of a waited-for slot whose batch asked for DELIVER_TRACE"""
        t = TraceDelivery()
        self._ck(self.L.hao_deliver_trace(self.h, slot, C.byref(t)), "hao_deliver_trace")
        return t

    def delivered_trace(self, d, rid, lengths=None):
        """(tasks uint32 [n,10], results int32 [n,6] (err, ps, pe, ts, te, cigar entries), cig_off uint64 [n+1], cigars uint16) of read rid's window pairs out of a
        Delivery with DELIVER_TRACE - fetch_trace_grid's shapes and values for the read (hao_unpack_trace; cig_off counts from the read's first entry)"""
        t, e = getattr(d, "tr", None), getattr(d, "ed", None)
        if t is None or e is None:
            raise HaoError("delivered_trace: the batch was not delivered with DELIVER_ED | DELIVER_TRACE")
        if lengths is None:
            lengths = getattr(self, "lengths", None)
        if lengths is None:
            raise HaoError("delivered_trace: the lengths of all reads are needed (pass lengths=)")
        L = np.ascontiguousarray(lengths, dtype=np.uint32)
        u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
        n = int(self.L.hao_unpack_trace(C.byref(t), C.byref(e), C.byref(d), L.ctypes.data_as(u32p), rid, None, None, None, None, 0, 0))
        co = _arr(t.cg_off + 8 * (rid - d.rid_lo), 2, np.uint64) if n else np.zeros(2, np.uint64)
        m = int(co[1] - co[0])
        tk = np.zeros((n, 10), dtype=np.uint32); r = np.zeros((n, 6), dtype=np.int32); off = np.zeros(n + 1, dtype=np.uint64); cg = np.zeros(max(m, 1), dtype=np.uint16)
        got = int(self.L.hao_unpack_trace(C.byref(t), C.byref(e), C.byref(d), L.ctypes.data_as(u32p), rid, tk.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p),
                                          off.ctypes.data_as(u64p), cg.ctypes.data_as(C.c_void_p), n, m))
        if got != n:
            raise HaoError(f"hao_unpack_trace: read {rid}: the pairs rebuilt from the delivered overlaps do not match the delivered counts (lengths of another read set?)")
        return tk, r, off, cg[:m]

    def delivered_read(self, d, rid):
        """(ol uint32 [n,12], fc uint64, fc_off uint64 [n+1], cl uint32 [m,4]) of read rid out of a Delivery view: what the h_ec_lchain shim hands to its caller"""
        r = rid - d.rid_lo
        oo = _arr(d.ol_off + 8 * r, 2, np.uint64)
        s_, e_ = int(oo[0]), int(oo[1])
        ol = np.zeros((e_ - s_, 12), dtype=np.uint32)                      # (the wire carries 32 of an overlap's 48 bytes)
        got = self.L.hao_unpack_overlaps(C.byref(d), rid, ol.ctypes.data_as(C.c_void_p), e_ - s_)
        assert got == e_ - s_
        lens = ol[:, 11].astype(np.int64)                                  # fc_len of every overlap; the cigars come through the decoder (the wire packs them)
        fo = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        fc = np.zeros(int(fo[-1]), dtype=np.uint64)
        for k in range(e_ - s_):
            got = self.L.hao_unpack_cigar(C.byref(d), s_ + k, fc[int(fo[k]):].ctypes.data_as(C.c_void_p), int(lens[k]))
            assert got == int(lens[k])
        co = _arr(d.cl_off + 8 * r, 2, np.uint64)
        m = int(co[1] - co[0])
        cl = np.zeros((m, 4), dtype=np.uint32)
        got = self.L.hao_unpack_hits(C.byref(d), rid, cl.ctypes.data_as(C.c_void_p), m)
        assert got == m
        return ol, fc, fo, cl

    def delivery_digest(self, d, threads=None):
        """hao_batch_digest's per-read value computed on the HOST from a delivered batch: ol, fake cigars, and cl->list decoded out of the wire format"""
        out = np.zeros(int(d.n_reads), dtype=np.uint64)
        self._ck(self.L.hao_delivery_digest(C.byref(d), out.ctypes.data_as(C.POINTER(C.c_uint64)), int(threads or min(32, os.cpu_count() or 1))), "hao_delivery_digest")
        return out

    def index_save(self, prefix, number_of_round=3, names=None):
        """write <prefix>.pt_flt / .pt_flt.bin / .pt_flt.paf.bin in the reference's resume format (write_pt_index, htab.cpp:1367).  On a sharded engine a
        collective: every rank calls it, rank 0 writes (it needs the gathered store, dist_gather_reads).  names: one str / bytes per GLOBAL read (rank 0's are read)"""
        arr = None
        if names is not None:
            arr = (C.c_char_p * len(names))(*[n if isinstance(n, bytes) else str(n).encode() for n in names])
        self._ck(self.L.hao_index_save(self.h, prefix.encode(), number_of_round, arr), "hao_index_save")

    def index_load(self, prefix, cuts=None):
        """hao_index_load / hao_index_load_dist: read store + filter table + position index from <prefix>.pt_flt[.bin] -> number_of_round stored in the file.
        On a sharded engine a collective; cuts: world + 1 first read ids in rank order (None: near-equal read counts).  n_reads, rid_base and lengths are
        set as set_readset and set_shard set them: the local reads' count and lengths, the global id of the first"""
        r = C.c_int32(0)
        if cuts is None:
            self._ck(self.L.hao_index_load(self.h, prefix.encode(), C.byref(r)), "hao_index_load")
        else:
            fr = np.ascontiguousarray(cuts, dtype=np.uint64)
            self._ck(self.L.hao_index_load_dist(self.h, prefix.encode(), fr.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(r)), "hao_index_load_dist")
        n, base, tot, al = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.POINTER(C.c_uint32)()
        self._ck(self.L.hao_shard_layout(self.h, C.byref(n), C.byref(base), C.byref(tot), C.byref(al)), "hao_shard_layout")
        self.n_reads, self.rid_base = int(n.value), int(base.value)
        self.lengths = _arr(al, tot.value, np.uint32)[self.rid_base:self.rid_base + self.n_reads]
        return r.value

    def window_trace_batch(self, tasks, cap=80, mode=0):
        """tasks: uint32 [n,10] -> (int32 [n,6] (err, ps, pe, ts, te, cigar entries), uint16 [n,cap] cigars): alignment in the band with traceback;
        mode 0 global (ed_band_cal_global_64_w_trace), 1 / 2 forward / backward extension (ed_band_cal_extension_64_{0,1}_w_trace), 3 semi-global with absent
        diagonals (ed_band_cal_semi_64_w_absent_diag_trace)"""
        t = np.ascontiguousarray(tasks, dtype=np.uint32).reshape(-1, 10)
        out = np.zeros((t.shape[0], 6), dtype=np.int32); cig = np.zeros((t.shape[0], cap), dtype=np.uint16)
        self._ck(self.L.hao_window_trace_batch(self.h, mode, t.ctypes.data_as(C.c_void_p), t.shape[0], out.ctypes.data_as(C.c_void_p), cig.ctypes.data_as(C.c_void_p), cap),
                 "hao_window_trace_batch")
        return out, cig

    def window_ed_batch(self, tasks):
        """tasks: uint32 [n,10] (p_rid, p_pos, p_len, p_rev, t_rid, t_pos, t_len, t_rev, thre, abs_diag) -> int32 [n,2] (err, pe)"""
        t = np.ascontiguousarray(tasks, dtype=np.uint32).reshape(-1, 10)
        out = np.zeros((t.shape[0], 2), dtype=np.int32)
        self._ck(self.L.hao_window_ed_batch(self.h, t.ctypes.data_as(C.c_void_p), t.shape[0], out.ctypes.data_as(C.c_void_p)), "hao_window_ed_batch")
        return out

    def window_ed_long(self, tasks):
        """window_ed_batch for thresholds up to 2047 and strings up to 16383 bases (bands of up to 64 words: the reference's *_infi_* functions); any mix of widths"""
        t = np.ascontiguousarray(tasks, dtype=np.uint32).reshape(-1, 10)
        out = np.zeros((t.shape[0], 2), dtype=np.int32)
        self._ck(self.L.hao_window_ed_long(self.h, t.ctypes.data_as(C.c_void_p), t.shape[0], out.ctypes.data_as(C.c_void_p)), "hao_window_ed_long")
        return out

    def window_trace_long(self, tasks, cap=80, mode=0):
        """window_trace_batch for thresholds up to 2047 and strings up to 16383 bases; same modes, records and cigar encoding"""
        t = np.ascontiguousarray(tasks, dtype=np.uint32).reshape(-1, 10)
        out = np.zeros((t.shape[0], 6), dtype=np.int32); cig = np.zeros((t.shape[0], cap), dtype=np.uint16)
        self._ck(self.L.hao_window_trace_long(self.h, mode, t.ctypes.data_as(C.c_void_p), t.shape[0], out.ctypes.data_as(C.c_void_p), cig.ctypes.data_as(C.c_void_p), cap),
                 "hao_window_trace_long")
        return out, cig

    def window_ladder(self, req, e_rate, maxl, maxe, cap=None):
        """hao_window_ladder over the current batch: req = LADDER_REQ records (or int rows ol, mode, qs, qe, ts, te, estimate_err) -> (LADDER_RES records, cig_off
        int64 [n + 1], cigars uint16).  cap = None: the stage runs once and the entries, which stay resident, are fetched at their size (hao_fetch_ladder); a
        number: the entries come back only when they fit it (cigars is None otherwise; cig_off[-1] is the capacity needed)"""
        return self._ladder(req, cap, LADDER_RES, "hao_window_ladder", self.L.hao_fetch_ladder,
                            lambda *a: self.L.hao_window_ladder(self.h, a[0], a[1], C.c_double(e_rate), C.c_int64(maxl), C.c_int64(maxe), *a[2:]))

    def window_ladder_adv(self, req, e_rate, wl, maxl, maxe, force_l, cap=None):
        """hao_window_ladder_adv (hc_aln_exz_adv's ladder: early returns, exact shortcut, five rungs, absolute coordinates) over the current batch; requests, cap and
        the returned triple as for window_ladder, the records being LADDER_ADV_RES; estimate_err = -1 asks for ql * e_rate (ql <= wl) or, on a longer stretch, for
        cal_estimate_err over the window lists the blocking chain (window_ed_ref, window_rescue_ref, window_wlist_ref) left on the device for the batch, built on this wl"""
        return self._ladder(req, cap, LADDER_ADV_RES, "hao_window_ladder_adv", self.L.hao_fetch_ladder_adv,
                            lambda *a: self.L.hao_window_ladder_adv(self.h, a[0], a[1], C.c_double(e_rate), C.c_int64(wl), C.c_int64(maxl), C.c_int64(maxe), C.c_int64(force_l), *a[2:]))

    @staticmethod
    def _ladder_req(req):
        q = np.asarray(req)
        if q.dtype != LADDER_REQ:
            rows = np.asarray(req, dtype=np.int64).reshape(-1, 7)
            q = np.zeros(rows.shape[0], dtype=LADDER_REQ)
            for k, f in enumerate(("ol", "mode", "qs", "qe", "ts", "te", "estimate_err")):
                q[f] = rows[:, k]
        return np.ascontiguousarray(q)

    def window_estimate_err(self, rows, e_rate, wl):
        """hao_window_estimate_err: cal_estimate_err over the window lists the blocking chain left on the device for the current batch, built on window length wl;
        rows = requests as for window_ladder_adv (ol, qs and qe are read) -> int64 [n], the function's value per request, a negative one included"""
        q = self._ladder_req(rows); n = q.shape[0]
        est = np.zeros(max(1, n), dtype=np.int64)
        self._ck(self.L.hao_window_estimate_err(self.h, q.ctypes.data_as(C.c_void_p), n, C.c_double(e_rate), C.c_int64(wl), est.ctypes.data_as(C.c_void_p)), "hao_window_estimate_err")
        return est[:n]

    def ladder_adv_estimates(self):
        """int64 [n]: the estimate each request of the last window_ladder_adv call ran with - its own where >= 0, ql * e_rate or the window lists' value where it
        was negative, -1 behind an early return (hao_fetch_ladder_adv_estimates)"""
        n = int(self.L.hao_fetch_ladder_adv_estimates(self.h, None, 0))
        if n >= 1 << 63:
            self._ck(n - (1 << 64), "hao_fetch_ladder_adv_estimates")
        est = np.zeros(max(1, n), dtype=np.int64)
        self.L.hao_fetch_ladder_adv_estimates(self.h, est.ctypes.data_as(C.c_void_p), n)
        return est[:n]

    def _ladder(self, req, cap, res_dtype, who, fetch, call):
        q = self._ladder_req(req); n = q.shape[0]
        res = np.zeros(n, dtype=res_dtype); off = np.zeros(n + 1, dtype=np.uint64); need = C.c_uint64()
        cig = np.zeros(max(1, cap or 0), dtype=np.uint16)
        self._ck(call(q.ctypes.data_as(C.c_void_p), n, res.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p), cig.ctypes.data_as(C.c_void_p), cap or 0, C.byref(need)), who)
        if cap is None:
            cig = np.zeros(max(1, need.value), dtype=np.uint16)
            self._ck(fetch(self.h, cig.ctypes.data_as(C.c_void_p), cig.shape[0], None, None), who + ": fetch")
            return res, off.astype(np.int64), cig[:need.value]
        return res, off.astype(np.int64), (cig[:need.value] if need.value <= cap else None)

    def ladder_rounds(self):
        """the requests that were open in each of the last hao_window_ladder call's four rounds"""
        r = (C.c_uint64 * 4)()
        self._ck(self.L.hao_fetch_ladder(self.h, None, 0, None, r), "hao_fetch_ladder")
        return [int(x) for x in r]

    def ladder_adv_rounds(self):
        """the requests that were open in each of the last hao_window_ladder_adv call's five rounds"""
        r = (C.c_uint64 * 5)()
        self._ck(self.L.hao_fetch_ladder_adv(self.h, None, 0, None, r), "hao_fetch_ladder_adv")
        return [int(x) for x in r]

    def window_ed_grid(self, window=375, thre=15):
        """window / candidate pairs of the last batch on the reference's window grid, generated and aligned on the device; returns their number"""
        n = C.c_uint64()
        self._ck(self.L.hao_window_ed_grid(self.h, C.c_uint32(window), C.c_uint32(thre), C.byref(n)), "hao_window_ed_grid")
        return int(n.value)

    def fetch_ed_grid(self, n):
        """(tasks uint32 [n,10], results int32 [n,2]) of the last hao_window_ed_grid"""
        t = np.zeros((n, 10), dtype=np.uint32); r = np.zeros((n, 2), dtype=np.int32)
        self._ck(self.L.hao_fetch_ed_grid(self.h, t.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), C.c_uint64(n)), "hao_fetch_ed_grid")
        return t, r

    def window_ed_ref(self, window=775, e_rate=0.04):
        """hao_window_ed_ref: the last batch's window / candidate pairs in REFERENCE placement, generated and aligned on the device; fetch_ed_grid serves tasks
        and results, fetch_ed_ovlp the per-overlap summaries.  Returns (pairs, unresolved windows)"""
        n, u = C.c_uint64(), C.c_uint64()
        self._ck(self.L.hao_window_ed_ref(self.h, C.c_uint32(window), C.c_double(e_rate), C.byref(n), C.byref(u)), "hao_window_ed_ref")
        return int(n.value), int(u.value)

    def fetch_ed_ovlp(self, rid):
        """uint32 [n_ol, 4] (windows covered, windows aligned, aligned bases, error sum) per overlap of read rid after window_ed_ref, aligned with h_ec_lchain(rid)[0]"""
        p, n = C.c_void_p(), C.c_uint64()
        self._ck(self.L.hao_fetch_ed_ovlp(self.h, rid, C.byref(p), C.byref(n)), "hao_fetch_ed_ovlp")
        return _arr(p.value, 4 * n.value, np.uint32).reshape(-1, 4)

    def window_rescue_ref(self):
        """hao_window_rescue_ref: the rescue of unaligned windows, the exit test and the verdict of align_hc_ed_post_extz over the batch window_ed_ref has
        just aligned; returns the number of rescued windows.  fetch_rescue serves the per-overlap results and the window records"""
        n = C.c_uint64()
        self._ck(self.L.hao_window_rescue_ref(self.h, C.byref(n)), "hao_window_rescue_ref")
        return int(n.value)

    def fetch_rescue(self, rid):
        """(ovlp, wins) of read rid after window_rescue_ref, aligned with h_ec_lchain(rid)[0]: ovlp = structured array (verdict, flags, exit_win, align_length,
        n_rescued) per overlap; wins = one int64 [m, 7] array per overlap (grid window, y_start, y_end, err, thre, direction, re-placed) in window order"""
        po, n, pw, pr = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_void_p()
        self._ck(self.L.hao_fetch_rescue(self.h, rid, C.byref(po), C.byref(n), C.byref(pw), C.byref(pr)), "hao_fetch_rescue")
        m = int(n.value)
        ov = _arr(po.value, m, RESCUE_OVLP)
        wo = _arr(pw.value, m + 1, np.uint64)
        wins = []
        for i in range(m):
            a, b = int(wo[i]), int(wo[i + 1])
            wins.append(rescue_records(_arr(pr.value + 16 * a, 4 * (b - a), np.uint32).reshape(-1, 4)))
        return ov, wins

    def deliver_wlist(self, slot):
        """the WlistDelivery view of a waited-for slot whose batch asked for DELIVER_WLIST"""
        w = WlistDelivery()
        self._ck(self.L.hao_deliver_wlist(self.h, slot, C.byref(w)), "hao_deliver_wlist")
        return w

    def delivered_wlist(self, d, rid, lengths=None):
        """the window lists of read rid out of a Delivery with DELIVER_ED | DELIVER_RESCUE | DELIVER_WLIST - fetch_wlist's shapes and values (hao_unpack_wlist)"""
        if getattr(d, "ed", None) is None or getattr(d, "rs", None) is None or getattr(d, "wl", None) is None:
            raise HaoError("delivered_wlist: the batch was not delivered with DELIVER_ED | DELIVER_RESCUE | DELIVER_WLIST")
        if lengths is None:
            raise HaoError("delivered_wlist: the lengths of all reads are needed (pass lengths=)")
        return unpack_wlist(d, d.ed, d.rs, d.wl, lengths, rid)

    def window_wlist_ref(self):
        """hao_window_wlist_ref: the window lists of the batch window_ed_ref and window_rescue_ref have just processed - every aligned window of every overlap
        with verdict 1, traced; returns (window records, windows swept, re-placement sweeps, cigar entries, untraced windows).  fetch_wlist serves them"""
        out = (C.c_uint64 * 5)()
        self._ck(self.L.hao_window_wlist_ref(self.h, out), "hao_window_wlist_ref")
        return tuple(int(x) for x in out)

    def fetch_wlist(self, rid):
        """the window lists of read rid after window_wlist_ref, aligned with h_ec_lchain(rid)[0]: one (wins, cigars) per overlap - wins = int64 [m, 8] (grid window,
        y_start, y_end, err, thre, source, re-placed, untraced) in window order, cigars = one uint16 array per record (push_trace's encoding; empty when untraced)"""
        n, pw, pr, po, pc = C.c_uint64(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._ck(self.L.hao_fetch_wlist(self.h, rid, C.byref(n), C.byref(pw), C.byref(pr), C.byref(po), C.byref(pc)), "hao_fetch_wlist")
        m = int(n.value)
        wo = _arr(pw.value, m + 1, np.uint64)
        nrec = int(wo[m])
        co = _arr(po.value, nrec + 1, np.uint64)
        return _wlist_split(wo, _arr(pr.value, 4 * nrec, np.uint32).reshape(-1, 4), co, _arr(pc.value, int(co[nrec]), np.uint16))

    def window_trace_grid(self, window=375, thre=15):
        """hao_window_trace_grid: the last batch's grid pairs aligned with traceback where they align inside the semi-global domain;
        returns (grid pairs, traced pairs, cigar entries, aligned but untraced pairs)"""
        out = (C.c_uint64 * 4)()
        self._ck(self.L.hao_window_trace_grid(self.h, C.c_uint32(window), C.c_uint32(thre), out), "hao_window_trace_grid")
        return tuple(int(x) for x in out)

    def fetch_trace_grid(self, n, n_cigar):
        """(tasks uint32 [n,10], results int32 [n,6] (err, ps, pe, ts, te, cigar entries), cig_off uint64 [n+1], cigars uint16 [n_cigar]) of the last
        hao_window_trace_grid: every grid pair, cigars in CSR form"""
        t = np.zeros((n, 10), dtype=np.uint32); r = np.zeros((n, 6), dtype=np.int32); off = np.zeros(n + 1, dtype=np.uint64); cg = np.zeros(max(n_cigar, 1), dtype=np.uint16)
        self._ck(self.L.hao_fetch_trace_grid(self.h, t.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.POINTER(C.c_uint64)),
                                             cg.ctypes.data_as(C.c_void_p), C.c_uint64(n), C.c_uint64(n_cigar)), "hao_fetch_trace_grid")
        return t, r, off, cg[:n_cigar]

    def fetch_exact(self, rid):
        """exact-overlap flags (uint8, aligned with h_ec_lchain(rid)[0]) of a read of the last batch"""
        p, n = C.c_void_p(), C.c_uint64()
        self._ck(self.L.hao_fetch_exact(self.h, rid, C.byref(p), C.byref(n)), "hao_fetch_exact")
        return _arr(p.value, n.value, np.uint8)

    def fetch_seed_hits(self, rid):
        p, n = C.c_void_p(), C.c_uint64()
        self._ck(self.L.hao_fetch_seed_hits(self.h, rid, C.byref(p), C.byref(n)), "hao_fetch_seed_hits")
        return _arr(p.value, 4 * n.value, np.uint32).reshape(-1, 4)

    def h_ec_lchain(self, rid):
        """-> (ol uint32 [n,12], fc uint64, fc_off uint64 [n+1], cl uint32 [m,4]) for a read of the last batch."""
        ol, fc, fo, cl = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        n, m = C.c_uint64(), C.c_uint64()
        self._ck(self.L.hao_fetch_overlaps(self.h, rid, C.byref(ol), C.byref(n), C.byref(fc), C.byref(fo), C.byref(cl), C.byref(m)),
                 "hao_fetch_overlaps")
        foff = _arr(fo.value, n.value + 1, np.uint64)
        nfc = int(foff[-1] - foff[0]) if foff.size else 0
        return (_arr(ol.value, 12 * n.value, np.uint32).reshape(-1, 12), _arr(fc.value, nfc, np.uint64), foff - (foff[0] if foff.size else 0),
                _arr(cl.value, 4 * m.value, np.uint32).reshape(-1, 4))

    def batch_totals(self):
        out = (C.c_uint64 * 8)()
        self._ck(self.L.hao_batch_totals(self.h, out), "hao_batch_totals")
        return dict(overlaps=int(out[0]), chained_hits=int(out[1]), seed_hits=int(out[2]), groups=int(out[3]), minimizers=int(out[4]), chains=int(out[5]),
                    seq_groups=int(out[6]), seq_group_hits=int(out[7]))

    def batch_seed_path(self):
        """which kernels carried the last batch's seed stage: (first launch: 2 list-major / 1 one-wave merge / 0 table kernels, reads left to the tables, 512- / 1024-slot overflows)"""
        out = (C.c_uint64 * 4)()
        self._ck(self.L.hao_batch_seed_path(self.h, out), "hao_batch_seed_path")
        return dict(first_launch={0: "seed_bin_kernel", 1: "(unused)", 2: "seed_lds_kernel"}[int(out[0])], left_to_tables=int(out[1]), overflow_512=int(out[2]), overflow_1024=int(out[3]))

    def batch_chain_path(self):
        """which kernels carried the last batch's chain stage: (groups per size class - up to 8 / 64 / 128 / 256 / 512 / 2048 hits and beyond -, and of those the groups
        the quick check handed to the DP kernel of their class), two lists of seven"""
        out = (C.c_uint64 * 16)()
        self._ck(self.L.hao_batch_chain_path(self.h, out), "hao_batch_chain_path")
        return [int(x) for x in out[0:7]], [int(x) for x in out[7:14]]

    def batch_digest(self, n, with_seed_hits=True):
        """per-read digests of the last batch (n reads): (digest of ol / fake cigars / cl, digest of the seed hits or None)"""
        d = np.zeros(n, dtype=np.uint64)
        k = np.zeros(n, dtype=np.uint64) if with_seed_hits else None
        u64p = C.POINTER(C.c_uint64)
        self._ck(self.L.hao_batch_digest(self.h, d.ctypes.data_as(u64p), k.ctypes.data_as(u64p) if k is not None else None), "hao_batch_digest")
        return d, k

    def stage_times(self):
        names = (C.c_char_p * 64)()
        ms = (C.c_float * 64)()
        n = self.L.hao_stage_times(self.h, names, ms, 64)
        return [(names[i].decode(), float(ms[i])) for i in range(n)]


def ladder_thresholds(ql, estimate_err, e_rate, maxl, maxe):
    """hao_ladder_thresholds: the four rungs' thresholds of a request as the device computes them (-1: skipped) and the number of attempts"""
    t = (C.c_int32 * 4)()
    n = lib().hao_ladder_thresholds(ql, estimate_err, C.c_double(e_rate), maxl, maxe, t)
    return [int(x) for x in t], n


def ladder_adv_thresholds(ql, estimate_err, e_rate, wl, maxl, maxe, force_l):
    """hao_ladder_adv_thresholds: the five raw rungs of hc_aln_exz_adv for a request as the device computes them (-1: skipped), whether the gate is open, and the
    number of attempts (negative: estimate_err < 0 with ql > wl)"""
    t = (C.c_int32 * 5)(); g = C.c_int32(0)
    n = lib().hao_ladder_adv_thresholds(ql, estimate_err, C.c_double(e_rate), wl, maxl, maxe, force_l, t, C.byref(g))
    return [int(x) for x in t], bool(g.value), n


def estimate_err_records(z, wins, wl, qs, qe, e_rate):
    """hao_estimate_err_records (host code): cal_estimate_err as the device computes it over one overlap z (a row of h_ec_lchain's overlap array) and its window
    records in ascending window order - fetch_wlist's int64 rows (grid window, y_start, y_end, err, ...) or raw hao_wlist_win_t words (uint32 [m, 4])"""
    w = np.asarray(wins)
    if w.dtype != np.uint32:
        w = np.asarray(wins, dtype=np.int64).reshape(-1, w.shape[1] if w.ndim == 2 and w.shape[0] else 8)
        raw = np.zeros((w.shape[0], 4), dtype=np.uint32)
        raw[:, 0] = w[:, 1].astype(np.uint32); raw[:, 1] = w[:, 2].astype(np.uint32); raw[:, 2] = w[:, 0]; raw[:, 3] = w[:, 3] & 0xff
        w = raw
    w = np.ascontiguousarray(w.reshape(-1, 4)); zz = np.ascontiguousarray(np.asarray(z, dtype=np.int64).astype(np.uint32))
    assert zz.shape == (12,)
    return int(lib().hao_estimate_err_records(zz.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), w.shape[0], int(wl), int(qs), int(qe), C.c_double(e_rate)))


def ref_thresholds(window, e_rate):
    """uint8 [window + 1]: the threshold of a window of q_l bases in reference placement (hao_ref_thresholds)"""
    out = np.zeros(int(window) + 1, dtype=np.uint8)
    lib().hao_ref_thresholds(C.c_uint32(window), C.c_double(e_rate), out.ctypes.data_as(C.POINTER(C.c_uint8)))
    return out
