"""ctypes binding of libstb_amd.so -- the C-ABI drop-in for libstb's S-table / sampler path.

Two layers, both thin:

* the reference's own interface (include/stable.h, psample.h, arms.h, yaps.h, sapprox.h), bound
  1:1 so that Python tests read like the reference's C callers (`S_make`, `S_S`, `samplea`, ...);
* the additive device interface (include/stb_hip.h) taking raw device pointers; `torch` is used
  here only to own HBM buffers and streams and to hand their addresses across the ABI.

There is no fallback of any kind: if the shared library is missing the import fails, and if no GPU
is present the library's entry points fail with a message (``stb_last_error``).
"""
from __future__ import annotations

import ctypes as C
import os
from functools import lru_cache

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("STB_LIB_PATH") or os.path.join(_HERE, "lib", "libstb_amd.so")

# flag bits of include/stable.h
S_STABLE, S_UVTABLE, S_FLOAT, S_VERBOSE, S_QUITONBOUND, S_THREADS, S_ASYMPT = 1, 2, 4, 8, 16, 32, 64
FILL_SCALED, FILL_LOGDOMAIN, FILL_SCALED_STEP, FILL_SPLIT, FILL_FUSED, FILL_PC, FILL_CHAIN, FILL_CHAINX, FILL_CK, FILL_HB = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9

c_double_p = C.POINTER(C.c_double)
c_u32_p = C.POINTER(C.c_uint32)
c_u16_p = C.POINTER(C.c_uint16)
c_int_p = C.POINTER(C.c_int)
c_float_p = C.POINTER(C.c_float)

LOGDENS = C.CFUNCTYPE(C.c_double, C.c_double, C.c_void_p)
GETVAL = C.CFUNCTYPE(None, c_u32_p, c_u16_p, C.c_uint, C.c_uint)


class StbError(RuntimeError):
    pass


JOINT_KEEP_L = 1  # stb_joint_opts_t flag: every stage's L values come back in the info (tests)


class JointOpts(C.Structure):
    """stb_joint_opts_t (include/stb_hip.h)"""
    _fields_ = [("a_lo", C.c_double), ("a_hi", C.c_double), ("b_lo", C.c_double), ("b_hi", C.c_double),
                ("D", C.c_int), ("J", C.c_int), ("shape", C.c_double), ("scale", C.c_double),
                ("seed", C.c_uint64), ("sweep", C.c_uint64), ("flags", C.c_uint)]


class ModeaInfo(C.Structure):
    """stb_modea_info_t (include/stb_hip.h)"""
    _fields_ = [("rounds", C.c_int), ("evals", C.c_int), ("at_bound", C.c_int), ("lo", C.c_double), ("hi", C.c_double),
                ("g_lo", C.c_double), ("g_hi", C.c_double), ("grad", C.c_double), ("delta", C.c_double)]


LJ_INDICATORS = 1  # stb_logjoint flag: the table-indicator representation (every pair also contributes -log C(n-1, t-1))


class LogJointInfo(C.Structure):
    """stb_logjoint_info_t (include/stb_hip.h)"""
    _fields_ = [("pairs", C.c_double), ("base", C.c_double), ("restaurants", C.c_double), ("binom", C.c_double),
                ("outside", C.c_uint64), ("impossible", C.c_uint64), ("t_mismatch", C.c_uint64)]


class TDishInfo(C.Structure):
    """stb_tdish_info_t (include/stb_hip.h)"""
    _fields_ = [("skipped", C.c_uint64), ("stuck", C.c_uint64)]


GH_ACCUMULATE = 1  # stb_gauss_heldout / stb_tindic_gauss_heldout flag: update the log-domain accumulator
PR_ACCUMULATE = 1  # stb_predict_dishes / stb_tindic_heldout flag: add the state's p into the accumulator


class PredictInfo(C.Structure):
    """stb_predict_info_t (include/stb_hip.h)"""
    _fields_ = [("skipped", C.c_uint64), ("impossible", C.c_uint64), ("customers", C.c_uint64)]


SEAT_COMMIT = 1  # stb_seat_customers flag: the one particle's seating is written back (n, t, T, cust, p)


class SeatInfo(C.Structure):
    """stb_seat_info_t (include/stb_hip.h)"""
    _fields_ = [("skipped", C.c_uint64), ("impossible", C.c_uint64), ("stuck", C.c_uint64), ("customers", C.c_uint64)]


class ClassesInfo(C.Structure):
    """stb_classes_info_t (include/stb_hip.h)"""
    _fields_ = [("skipped", C.c_uint64), ("stuck", C.c_uint64), ("drawn", C.c_uint64)]


class GaussPrior(C.Structure):
    """stb_gauss_prior_t (include/stb_hip.h)"""
    _fields_ = [("kappa0", C.c_double), ("alpha0", C.c_double), ("beta00", C.c_double),
                ("m0", C.POINTER(C.c_double)), ("beta0", C.POINTER(C.c_double))]


class GaussInfo(C.Structure):
    """stb_gauss_info_t (include/stb_hip.h)"""
    _fields_ = [("skipped", C.c_uint64), ("dead", C.c_uint64)]


GS_MAXD = 64  # STB_GS_MAXD
PF_MAXR = 64  # STB_PF_MAXR: the slots of stb_seat_filter, a slot a lane


class PFInfo(C.Structure):
    """stb_pf_info_t (include/stb_hip.h)"""
    _fields_ = [("skipped", C.c_uint64), ("impossible", C.c_uint64), ("stuck", C.c_uint64), ("dead", C.c_uint64),
                ("resamplings", C.c_uint64), ("customers", C.c_uint64)]


GEOM_LOGQ, GEOM_JOINT_TERMS, GEOM_LOGJOINT = 0, 1, 2  # stb_reduce_geometry's `which`


class AISInfo(C.Structure):
    """stb_ais_info_t (include/stb_hip.h)"""
    _fields_ = [("skipped", C.c_uint64), ("dead", C.c_uint64), ("stuck", C.c_uint64), ("customers", C.c_uint64)]


class ReduceGeom(C.Structure):
    """stb_reduce_geom_t (include/stb_hip.h)"""
    _fields_ = [("grid_x", C.c_uint), ("grid_y", C.c_uint), ("steps", C.c_uint), ("chunks", C.c_uint),
                ("blocks", C.c_uint), ("waves", C.c_uint), ("need", C.c_uint64), ("cap0", C.c_uint64)]


class BGroupsInfo(C.Structure):
    """stb_bgroups_info_t (include/stb_hip.h)"""
    _fields_ = [("bad_restaurants", C.c_uint64), ("kept_groups", C.c_uint64), ("error_word", C.c_uint),
                ("reserved", C.c_uint), ("b", C.c_double)]


HG_KEEP_ROOT = 1      # stb_hgroups_opts_t flags (include/stb_hip.h)
HG_SAMPLE_ALPHA = 2


class HGroupsOpts(C.Structure):
    """stb_hgroups_opts_t (include/stb_hip.h)"""
    _fields_ = [("alpha", C.c_double), ("gamma0", C.c_double), ("shape", C.c_double), ("scale", C.c_double),
                ("gamma_host", c_double_p), ("flags", C.c_uint), ("reserved", C.c_uint)]


class HGroupsInfo(C.Structure):
    """stb_hgroups_info_t (include/stb_hip.h)"""
    _fields_ = [("alpha", C.c_double), ("tables", C.c_uint64), ("aux_tables", C.c_uint64), ("error_word", C.c_uint),
                ("reserved", C.c_uint)]


HT_MAXL = 8           # STB_HT_MAXL
HT_KEEP_ROOT = 1      # stb_htree_opts_t flags (include/stb_hip.h)
HT_SAMPLE_ALPHA = 2


class HTreeOpts(C.Structure):
    """stb_htree_opts_t (include/stb_hip.h)"""
    _fields_ = [("levels", C.c_int), ("alpha", c_double_p), ("gamma0", C.c_double), ("shape", C.c_double), ("scale", C.c_double),
                ("gamma_host", c_double_p), ("flags", C.c_uint), ("reserved", C.c_uint)]


class HTreeInfo(C.Structure):
    """stb_htree_info_t (include/stb_hip.h)"""
    _fields_ = [("alpha", C.c_double * HT_MAXL), ("tables", C.c_uint64 * HT_MAXL), ("aux_tables", C.c_uint64 * HT_MAXL),
                ("error_word", C.c_uint), ("reserved", C.c_uint)]


DM_ROWS, DM_COLUMNS = 1, 2  # stb_dirmult_logml's orientation: a multinomial a row / a column


class DirMultInfo(C.Structure):
    """stb_dirmult_info_t (include/stb_hip.h)"""
    _fields_ = [("cells", C.c_double), ("norms", C.c_double), ("nonzero", C.c_uint64), ("count", C.c_uint64),
                ("zero_weight", C.c_uint64), ("impossible", C.c_uint64), ("error_word", C.c_uint), ("reserved", C.c_uint)]


class DirConcInfo(C.Structure):
    """stb_dirconc_info_t (include/stb_hip.h)"""
    _fields_ = [("s", C.c_double), ("count", C.c_uint64), ("aux_tables", C.c_uint64), ("nonempty", C.c_uint64),
                ("zero_weight", C.c_uint64), ("error_word", C.c_uint), ("reserved", C.c_uint)]


CJ_INDICATORS, CJ_FLAT, CJ_DATA, CJ_ROOT = 1, 2, 4, 8  # stb_tindic_logjoint_collapsed's flags


class CJOpts(C.Structure):
    """stb_cj_opts_t (include/stb_hip.h)"""
    _fields_ = [("alpha", C.c_double), ("gamma0", C.c_double), ("beta0", C.c_double), ("gamma_host", c_double_p),
                ("beta_host", c_double_p)]


class CJInfo(C.Structure):
    """stb_cj_info_t (include/stb_hip.h)"""
    _fields_ = [("pairs", C.c_double), ("restaurants", C.c_double), ("binom", C.c_double), ("tables", C.c_double),
                ("data", C.c_double), ("root", C.c_double), ("lj", LogJointInfo), ("dm_tables", DirMultInfo),
                ("dm_data", DirMultInfo), ("root_left_out", C.c_uint64)]


class JointInfo(C.Structure):
    """stb_joint_info_t (include/stb_hip.h)"""
    _fields_ = [("stages", C.c_int), ("accepted", C.c_int), ("evals", C.c_int), ("stage_pick", C.c_int),
                ("log_alpha", C.c_double), ("rect", C.c_double * 4), ("a_prop", C.c_double), ("b_prop", C.c_double),
                ("L_cur", C.c_double), ("L_prop", C.c_double), ("cell", C.c_int * 5), ("box", (C.c_int * 4) * 5),
                ("L", c_double_p)]


@lru_cache(maxsize=None)
def lib() -> C.CDLL:
    if not os.path.exists(LIB_PATH):
        raise StbError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C libstb_amd/csrc` (there is no pure-Python or CPU implementation)")
    # torch ships its own libamdhip64.so.7; libstb_amd.so needs the same SONAME.  Whichever is
    # loaded first serves both, and two HIP runtimes in one process do not see the GPU reliably,
    # so when torch is importable it goes first and this library runs on torch's runtime (plain
    # C callers get the system ROCm runtime instead).
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch-less environments
        pass
    L = C.CDLL(LIB_PATH)
    u, d, i, vp, u64, sz = C.c_uint, C.c_double, C.c_int, C.c_void_p, C.c_uint64, C.c_size_t

    # entry points added in round 5: an older build loaded through STB_LIB_PATH (tools/ab_lib.py, A/B against an
    # earlier round's library) simply lacks them; everything else must be there
    ROUND5 = {"stb_groups_pairs_begin", "stb_groups_pairs_put", "stb_groups_pairs_put_ragged", "stb_groups_pairs_commit",
              "stb_groups_update_pairs", "stb_groups_fallbacks", "stb_grid_shape", "stb_bterms_update",
              # ... and in round 6
              "stb_table_probe", "stb_slow_launches", "stb_shared_gpu_mode", "stb_set_shared_gpu", "stb_note_launch_span",
              "stb_lookup_V", "stb_lookup_U", "stb_lookup_UV", "stb_groups_aterms_multi", "stb_groups_create_node",
              # ... and the diagnostics of the truth tests at working shapes
              "stb_groups_last_form"}

    def sig(name, res, args):
        try:
            f = getattr(L, name)
        except AttributeError:
            if name in ROUND5 and os.environ.get("STB_LIB_PATH"):
                return
            raise
        f.restype = res
        f.argtypes = args

    # ---- include/stable.h
    sig("S_make", vp, [u, u, u, u, d, C.c_uint32])
    sig("S_tag", None, [vp, C.c_char_p])
    sig("S_remake", i, [vp, d])
    sig("S_free", None, [vp])
    for n in ("S_S", "S_U", "S_UV", "S_V", "S_asympt"):
        sig(n, d, [vp, u, u])
    sig("S_S1", d, [vp, u])
    sig("S_report", None, [vp, vp])
    sig("stb_extend_policy", None, [u, u, u, u, i, i, C.POINTER(u), C.POINTER(u)])
    sig("stb_table_sync", i, [vp])
    sig("stb_table_probe", None, [vp, i, C.POINTER(u), C.POINTER(u), sz, c_double_p])
    sig("stb_table_mirrored", None, [vp, C.POINTER(u), C.POINTER(u)])
    sig("stb_table_bytes", None, [vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)])
    # ---- include/yaps.h
    sig("yaps_yapper", None, [vp])
    # ---- include/stb_hip.h
    sig("stb_last_error", C.c_char_p, [])
    sig("stb_device_count", i, [])
    sig("stb_device_name", i, [C.c_char_p, i])
    sig("stb_set_device", i, [i])
    sig("stb_get_device", i, [])
    sig("stb_device_enter", i, [i])
    sig("stb_device_leave", None, [i])
    sig("stb_device_malloc", vp, [sz])
    sig("stb_device_free", None, [vp])
    sig("stb_host_malloc", vp, [sz])
    sig("stb_host_free", None, [vp])
    sig("stb_memcpy_h2d", i, [vp, vp, sz, vp])
    sig("stb_memcpy_d2h", i, [vp, vp, sz, vp])
    sig("stb_stream_sync", i, [vp])
    for n in ("stb_cells", "stb_elems", "stb_vcells", "stb_velems"):
        sig(n, u64, [u, u])
    sig("stb_rowoff", u64, [u, u])
    sig("stb_vrowoff", u64, [u, u])
    sig("stb_fill_workspace_bytes", sz, [u, u, i])
    sig("stb_default_variant", i, [])
    sig("stb_fill_S", i, [c_double_p, i, u, u, vp, u64, vp, u64, vp, sz, i, vp])
    sig("stb_fill_tuning", i, [u, u, i, c_int_p, c_int_p, c_int_p])
    sig("stb_fill_status", i, [])
    sig("stb_fill_fallbacks", C.c_uint, [])
    sig("stb_has_ablation", i, [])
    sig("stb_slow_launches", C.c_uint, [])
    sig("stb_shared_gpu_mode", i, [])
    sig("stb_set_shared_gpu", None, [i])
    sig("stb_note_launch_span", None, [C.c_double, C.c_double])
    sig("stb_fill_profile_begin", None, [])
    sig("stb_fill_profile_end", i, [c_double_p, c_int_p])
    sig("stb_fill_profile_span", C.c_double, [])
    sig("stb_fill_V", i, [c_double_p, i, u, u, vp, u64, vp, sz, vp])
    sig("stb_fill_V_exact", i, [c_double_p, i, u, u, vp, u64, vp, sz, vp])
    sig("stb_fill_Vf", i, [c_double_p, i, u, u, vp, u64, vp, sz, vp])
    sig("stb_fill_Sf", i, [c_double_p, i, u, u, vp, u64, vp, u64, vp, sz, vp])
    sig("stb_fill_takes_kind", i, [u, u, i, i])
    sig("stb_bterms_create", vp, [c_u32_p, i])
    sig("stb_bterms_update", i, [vp, c_u32_p, i])
    sig("stb_bterms_eval", i, [vp, c_double_p, i, d, d, d, c_double_p])
    sig("stb_bterms_free", None, [vp])
    sig("stb_table_to_float", i, [vp, vp, u64, vp])
    sig("stb_lookup_S", i, [vp, vp, u, u, vp, vp, u64, vp, vp])
    sig("stb_lookup_V", i, [vp, u, u, vp, vp, u64, vp, vp])
    sig("stb_lookup_U", i, [vp, u, u, C.c_double, vp, vp, u64, vp, vp])
    sig("stb_lookup_UV", i, [vp, u, u, C.c_double, vp, vp, u64, vp, vp])
    sig("stb_sweep_workspace_bytes", sz, [u64, i])
    sig("stb_sweep_S", i, [vp, u64, vp, u64, i, u, u, vp, vp, u64, vp, vp, sz, vp])
    sig("stb_terms_workspace_bytes", sz, [u64, i])
    sig("stb_restaurant_terms", i, [c_double_p, i, vp, vp, u64, vp, vp, sz, vp])
    sig("stb_bterms", i, [c_double_p, i, d, d, d, vp, u64, vp, vp, sz, vp])
    sig("stb_groups_create", vp, [i, c_int_p, c_u32_p, c_u32_p, c_u16_p, c_double_p, u, u, i])
    sig("stb_groups_free", None, [vp])
    sig("stb_groups_aterms", i, [vp, c_double_p, i, c_double_p])
    sig("stb_groups_aterms_tables", i, [vp, c_double_p, i, c_double_p])
    sig("stb_groups_aterms_async", i, [vp, c_double_p, i, c_double_p, vp])
    sig("stb_groups_wait", i, [vp])
    sig("stb_groups_aterms_multi", i, [C.POINTER(vp), i, c_double_p, i, c_double_p])
    sig("stb_groups_create_node", i, [i, i, c_int_p, c_u32_p, c_u32_p, c_u16_p, c_double_p, u, u, i, C.POINTER(vp)])
    sig("stb_groups_aterms_device", i, [vp, c_double_p, i, vp, vp])
    sig("stb_groups_update_restaurants", i, [vp, c_u32_p, c_double_p])
    sig("stb_groups_pairs_begin", i, [vp])
    sig("stb_groups_pairs_put", i, [vp, c_u32_p, c_u16_p, u64, C.POINTER(u), C.POINTER(u)])
    sig("stb_groups_pairs_put_ragged", i, [vp, i, c_int_p, vp, vp, C.POINTER(u), C.POINTER(u)])
    sig("stb_groups_pairs_commit", i, [vp, c_u32_p, c_double_p, u, u])
    sig("stb_groups_update_pairs", i, [vp, c_u32_p, c_u16_p])
    sig("stb_groups_fallbacks", C.c_uint, [])
    sig("stb_grid_shape", i, [u, u, i, c_int_p, c_int_p, c_int_p])
    sig("stb_groups_shape", i, [vp, c_int_p, C.POINTER(u64), C.POINTER(u), C.POINTER(u), c_int_p])
    sig("stb_groups_last_form", i, [vp, c_int_p, c_int_p, c_int_p, c_int_p, c_int_p])
    sig("stb_sampler_cache_clear", None, [])
    sig("stb_groups_aterms_timed", i, [vp, c_double_p, i, c_double_p, c_float_p, c_float_p, c_float_p])
    sig("stb_sample_tcounts", i, [vp, vp, u, u, d, vp, i, vp, vp, vp, vp, vp, u64, u64, vp])
    sig("stb_tcounts_create", vp, [i, c_int_p, c_u32_p, c_u16_p, c_double_p, u])
    sig("stb_tcounts_set_h", i, [vp, c_double_p])
    sig("stb_tcounts_sweep", i, [vp, d, c_double_p, u64, u64, i])
    sig("stb_tcounts_get", i, [vp, c_u16_p, c_u32_p])
    sig("stb_tcounts_to_groups", i, [vp, vp, c_double_p])
    sig("stb_tcounts_free", None, [vp])
    sig("stb_sample_tcounts_window", i, [vp, vp, u, u, d, vp, i, vp, vp, vp, vp, vp, u, u, u64, u64, vp])
    sig("stb_tcounts_sweep_window", i, [vp, d, c_double_p, u, u, u64, u64, i])
    sig("stb_sample_tindic", i, [vp, u, u, d, vp, i, vp, vp, vp, vp, vp, vp, vp, u, u64, u64, vp])
    sig("stb_tindic_create", vp, [i, c_int_p, c_u32_p, c_u16_p, c_double_p, c_u32_p, u, u])
    sig("stb_tindic_set_h", i, [vp, c_double_p])
    sig("stb_tindic_sweep", i, [vp, d, c_double_p, u64, u64, i])
    sig("stb_tindic_get", i, [vp, c_u16_p, c_u32_p])
    sig("stb_tindic_to_groups", i, [vp, vp, c_double_p])
    sig("stb_tindic_free", None, [vp])
    sig("stb_sample_tdishes", i, [vp, u, u, d, vp, i, vp, vp, vp, vp, vp, vp, vp, vp, vp, u, u, u64, u64, vp, vp])
    sig("stb_tindic_set_classes", i, [vp, c_u32_p, u])
    sig("stb_tindic_set_lik", i, [vp, c_double_p, u, u])
    sig("stb_tindic_lik_device", vp, [vp, C.POINTER(u), C.POINTER(u), C.POINTER(vp)])
    sig("stb_tindic_sweep_dishes", i, [vp, d, c_double_p, u64, u64, i, C.POINTER(TDishInfo)])
    sig("stb_tindic_get_state", i, [vp, c_u32_p, c_u32_p])
    sig("stb_tindic_class_counts", i, [vp, c_u32_p])
    # ---- the likelihood and the base weights drawn on the device, the data term
    sig("stb_sample_lik", i, [vp, u, u, c_double_p, d, vp, u64, u64, vp])
    sig("stb_lik_loglik", i, [vp, vp, u, u, c_double_p, C.POINTER(u64), vp])
    sig("stb_tindic_sample_lik", i, [vp, c_double_p, d, u64, u64])
    sig("stb_tindic_sample_h", i, [vp, c_double_p, d, u64, u64])
    sig("stb_tindic_loglik", i, [vp, c_double_p, C.POINTER(u64)])
    sig("stb_tindic_get_h", i, [vp, c_double_p])
    # ---- base weights per group of restaurants under a shared root
    hgo, hgi = C.POINTER(HGroupsOpts), C.POINTER(HGroupsInfo)
    sig("stb_sample_hgroups", i, [i, vp, vp, u, i, vp, hgo, vp, vp, vp, vp, vp, u64, u64, vp, hgi])
    sig("stb_tindic_set_hgroups", i, [vp, i, C.POINTER(u64)])
    sig("stb_tindic_set_hroot", i, [vp, c_double_p])
    sig("stb_tindic_get_hroot", i, [vp, c_double_p])
    sig("stb_tindic_sample_hgroups", i, [vp, hgo, u64, u64, hgi])
    hto, hti, vpp = C.POINTER(HTreeOpts), C.POINTER(HTreeInfo), C.POINTER(C.c_void_p)
    sig("stb_sample_htree", i, [i, vp, vp, u, C.POINTER(i), vpp, hto, vp, vpp, vp, vpp, vpp, u64, u64, vp, hti])
    sig("stb_tindic_set_htree", i, [vp, i, C.POINTER(i), vpp])
    sig("stb_tindic_set_htree_level", i, [vp, i, c_double_p])
    sig("stb_tindic_get_htree_level", i, [vp, i, c_double_p])
    sig("stb_tindic_sample_htree", i, [vp, hto, u64, u64, hti])
    sig("stb_sample_partition", i, [vp, vp, u, u, d, u64, vp, vp, vp, u, vp, vp, u, u64, u64, vp])
    sig("stb_tcounts_partition", i, [vp, d, vp, c_double_p, u64, u64])
    sig("stb_hist_create_empty", vp, [u, i])
    sig("stb_hist_restaurants", i, [vp, c_u32_p, c_double_p])
    sig("stb_hist_counts_device", vp, [vp, C.POINTER(u), C.POINTER(vp)])
    sig("stb_hist_get", i, [vp, c_u32_p])
    sig("stb_bterms_borrow", vp, [vp, vp, i, vp])
    sig("stb_sample_logq", i, [d, d, i, vp, vp, c_double_p, u64, u64, vp])
    sig("stb_sampleb_device", d, [d, i, d, d, vp, vp, d, vp, i, i, u64, u64, vp])
    sig("stb_tcounts_sampleb", d, [vp, d, d, d, d, vp, i, i, u64, u64])
    sig("stb_tindic_sampleb", d, [vp, d, d, d, d, vp, i, i, u64, u64])
    sig("stb_sampleb_last_Q", d, [])
    # ---- one concentration per group of restaurants, drawn on the device
    bgi = C.POINTER(BGroupsInfo)
    sig("stb_sample_bgroups", i, [d, d, d, i, vp, vp, vp, i, vp, vp, vp, vp, vp, u64, u64, vp, bgi])
    sig("stb_hb_bgroups", i, [d, d, d, i, vp, vp, vp, i, vp, vp, vp, vp, vp, vp, u64, u64, vp, bgi, C.c_char_p])
    for obj in ("tcounts", "tindic"):
        sig("stb_%s_set_bpar" % obj, i, [vp, c_double_p])
        sig("stb_%s_get_bpar" % obj, i, [vp, c_double_p])
        sig("stb_%s_set_bgroups" % obj, i, [vp, i, C.POINTER(u64)])
        sig("stb_%s_sampleb_groups" % obj, i, [vp, d, d, d, u64, u64, c_double_p, bgi])
    sig("stb_groups_samplea", d, [vp, d, vp, i, i])
    sig("stb_groups_ssum", i, [vp, c_double_p, i, c_double_p])
    sig("stb_groups_ssum_device", i, [vp, c_double_p, i, vp, vp])
    sig("stb_joint_terms", i, [c_double_p, i, c_double_p, i, vp, vp, u64, vp, vp])
    jo, ji = C.POINTER(JointOpts), C.POINTER(JointInfo)
    sig("stb_groups_samplejoint", i, [vp, vp, jo, d, d, c_double_p, c_double_p, ji])
    sig("stb_tcounts_samplejoint", i, [vp, vp, jo, d, d, c_double_p, c_double_p, ji])
    sig("stb_tindic_samplejoint", i, [vp, vp, jo, d, d, c_double_p, c_double_p, ji])
    # ---- the log joint of a sampler state
    lji = C.POINTER(LogJointInfo)
    sig("stb_logjoint", i, [vp, vp, u, u, d, vp, i, vp, vp, vp, vp, vp, u, vp, c_double_p, lji, vp])
    sig("stb_tcounts_logjoint", i, [vp, d, c_double_p, u, c_double_p, c_double_p, lji])
    sig("stb_tindic_logjoint", i, [vp, d, c_double_p, u, c_double_p, c_double_p, lji])
    sig("stb_dirmult_logml", i, [vp, u64, u, u, u, vp, d, d, vp, vp, c_double_p, C.POINTER(DirMultInfo), vp])
    sig("stb_tindic_logjoint_collapsed", i, [vp, d, c_double_p, u, C.POINTER(CJOpts), c_double_p, C.POINTER(CJInfo)])
    dci = C.POINTER(DirConcInfo)
    sig("stb_sample_dirconc", i, [vp, u64, u, u, u, vp, d, d, d, d, vp, vp, u64, u64, vp, dci])
    sig("stb_tindic_sample_beta", i, [vp, c_double_p, d, d, d, u64, u64, dci])
    sig("stb_tindic_sample_gamma", i, [vp, c_double_p, d, d, d, u64, u64, dci])
    sig("stb_reduce_geometry", i, [i, u64, i, i, i, C.POINTER(ReduceGeom)])
    # ---- what a state predicts: dish proportions and held-out customers
    pri = C.POINTER(PredictInfo)
    sig("stb_predict_dishes", i, [d, vp, i, vp, vp, vp, vp, vp, u, vp, vp, vp, u, u, vp, u, vp, vp])
    sig("stb_heldout_loglik", i, [vp, vp, i, u, vp, c_double_p, pri, vp])
    sig("stb_tindic_set_heldout", i, [vp, C.POINTER(u64), c_u32_p])
    sig("stb_tindic_predict", i, [vp, d, c_double_p, c_double_p, u])
    sig("stb_tindic_heldout", i, [vp, d, c_double_p, u, c_double_p, c_double_p, pri])
    sig("stb_tindic_heldout_reset", i, [vp])
    sig("stb_tindic_heldout_get", i, [vp, c_double_p, C.POINTER(u)])
    # ---- seating customers one by one
    sti = C.POINTER(SeatInfo)
    sig("stb_seat_customers", i, [d, vp, i, vp, vp, vp, vp, vp, u, vp, vp, vp, vp, u, u, u, u, u64, u64, vp, vp, vp, vp])
    sig("stb_seat_loglik", i, [vp, i, u, vp, c_double_p, sti, vp])
    sig("stb_tindic_seat", i, [vp, d, c_double_p, u64, u64, c_double_p, sti])
    sig("stb_tindic_heldout_seq", i, [vp, d, c_double_p, u, u64, u64, c_double_p, c_double_p, sti])
    # ---- the seating as a particle filter
    sig("stb_seat_filter", i, [d, vp, i, vp, vp, vp, vp, u, vp, vp, vp, u, u, u, d, u64, u64, vp, vp, vp, vp, vp, vp, vp, vp])
    sig("stb_seat_filter_budget", u, [u])
    sig("stb_tindic_heldout_pf", i, [vp, d, c_double_p, u, d, u64, u64, c_double_p, c_double_p, C.POINTER(PFInfo)])
    # ---- annealed importance sampling
    sig("stb_seat_anneal_workspace_bytes", C.c_size_t, [i, u64, u64, u, u, u])
    sig("stb_lik_temper", i, [vp, u, u, d, vp, vp])
    sig("stb_seat_anneal", i, [vp, u, u, d, vp, i, vp, vp, vp, vp, vp, u, u, u64, u64, u, u, c_double_p, u, u64, u64, vp, vp, vp,
                               vp, vp, vp, C.c_size_t, vp])
    sig("stb_tindic_heldout_ais", i, [vp, d, c_double_p, u, u, c_double_p, u, u64, u64, c_double_p, c_double_p,
                                      C.POINTER(AISInfo)])
    # ---- customers' classes drawn on the device
    cli = C.POINTER(ClassesInfo)
    sig("stb_sample_classes", i, [vp, u, u, vp, vp, u64, u64, u64, vp, vp, vp])
    sig("stb_tindic_sample_classes", i, [vp, vp, u64, u64, cli])
    sig("stb_tindic_generate", i, [vp, d, c_double_p, u64, u64, sti, cli])
    sig("stb_tindic_get_classes", i, [vp, c_u32_p, C.POINTER(u)])
    # ---- Gaussian observations
    gsp, gsi = C.POINTER(GaussPrior), C.POINTER(GaussInfo)
    sig("stb_gauss_stats", i, [vp, u, vp, u64, u, vp, vp, vp, gsi, vp])
    sig("stb_sample_gauss", i, [vp, vp, vp, u, u, gsp, u64, u64, vp, vp, vp])
    sig("stb_gauss_lik", i, [vp, u, u64, vp, vp, u, vp, u, gsi, vp])
    sig("stb_gauss_loglik", i, [vp, u, vp, u64, vp, vp, u, c_double_p, gsi, vp])
    sig("stb_gauss_logml", i, [vp, vp, vp, u, u, gsp, c_double_p, vp])
    sig("stb_tindic_set_obs", i, [vp, c_double_p, u])
    sig("stb_tindic_set_gauss", i, [vp, c_double_p, c_double_p])
    sig("stb_tindic_get_gauss", i, [vp, c_double_p, c_double_p])
    sig("stb_tindic_sample_gauss", i, [vp, gsp, u64, u64, gsi])
    sig("stb_tindic_gauss_loglik", i, [vp, c_double_p])
    sig("stb_tindic_gauss_logml", i, [vp, gsp, c_double_p])
    # ---- held-out points under Gaussian observations
    sig("stb_gauss_heldout", i, [vp, u, i, vp, vp, u, vp, vp, u, vp, vp, u, vp, vp, u, vp])
    sig("stb_gauss_heldout_loglik", i, [vp, vp, vp, u, vp, i, vp, c_double_p, pri, vp])
    sig("stb_tindic_set_heldout_obs", i, [vp, C.POINTER(u64), c_double_p])
    sig("stb_tindic_gauss_heldout", i, [vp, d, c_double_p, u, c_double_p, c_double_p, c_double_p, pri])
    sig("stb_tindic_gauss_heldout_reset", i, [vp])
    sig("stb_tindic_gauss_heldout_get", i, [vp, c_double_p, c_double_p, C.POINTER(u)])
    # (private entry points: the customers per restaurant as d_N or as d_coff prefix sums, for tests)
    sig("stb_hq_logq", i, [d, d, i, vp, vp, vp, c_double_p, u64, u64, vp])
    sig("stb_hj_joint_terms", i, [c_double_p, i, c_double_p, i, vp, vp, vp, u64, vp, vp])
    # ---- the slope of log S in the discount
    sig("stb_fill_dS_workspace_bytes", sz, [u, u, i])
    sig("stb_fill_dS", i, [c_double_p, i, u, u, vp, u64, vp, u64, vp, u64, vp, u64, vp, sz, vp])
    sig("stb_fill_dS_geometry", None, [u, c_int_p, c_int_p, c_int_p, c_int_p, c_int_p])
    sig("stb_lookup_dS", i, [vp, vp, u, u, vp, vp, u64, vp, vp])
    sig("stb_sweep_dS", i, [vp, u64, vp, u64, i, u, u, vp, vp, u64, vp, vp, sz, vp])
    sig("stb_restaurant_terms_da", i, [c_double_p, i, vp, vp, u64, vp, vp, sz, vp])
    sig("stb_groups_aterms_grad", i, [vp, c_double_p, i, c_double_p, c_double_p])
    sig("stb_groups_modea", i, [vp, d, d, d, i, c_double_p, c_double_p, C.POINTER(ModeaInfo)])
    # optional entry points (present once the sampler host code is linked in)
    for name, res, args in (
        ("arms_simple", i, [i, c_double_p, c_double_p, LOGDENS, vp, i, c_double_p, c_double_p]),
        ("arms", i, [c_double_p, i, c_double_p, c_double_p, LOGDENS, vp, c_double_p, i, i, c_double_p,
                     c_double_p, i, c_double_p, c_double_p, i, c_int_p]),
        ("expshift", d, [d, d]),
        ("SliceSimple", i, [c_double_p, LOGDENS, c_double_p, vp, i, vp]),
        ("samplea", d, [d, i, c_int_p, c_u32_p, C.POINTER(c_u32_p), C.POINTER(c_u16_p), vp, c_double_p,
                        vp, i, i]),
        ("sampleb", d, [d, i, d, d, c_u32_p, c_u32_p, d, vp, i, i]),
        ("samplea2", d, [d, vp, i, c_int_p, c_u32_p, C.POINTER(c_u32_p), C.POINTER(c_u16_p), vp, c_double_p, vp, i, i]),
        ("stb_samplea2_partition", sz, [C.POINTER(c_u16_p)]),
        ("stb_hist_create", vp, [c_u32_p, u, i, c_u32_p, c_double_p]),
        ("stb_hist_aterms2", i, [vp, c_double_p, i, c_double_p]),
        ("stb_hist_free", None, [vp]),
        ("stb_samplea2_hist", d, [d, vp, vp, i, i]),
        ("S_approx", d, [i, i, C.c_float]),
        ("S_approx_da", d, [i, i, C.c_float]),
        ("digammaRN", d, [d]),
        ("gsl_rng_gamma", d, [d]),
        ("gsl_rng_beta", d, [d, d]),
        ("gsl_rng_gaussian_ziggurat", d, [d]),
        ("stb_sampler_trace_count", i, []),
        ("stb_sampler_trace_get", i, [i, c_double_p, c_double_p]),
        ("stb_sampler_trace_code", i, []),
        ("stb_zig_table", d, [i, i]),
    ):
        if hasattr(L, name):
            sig(name, res, args)
    return L


ABLATION_VARIANTS = (FILL_SCALED_STEP, FILL_SPLIT, FILL_FUSED, FILL_CHAINX)


def has_variant(variant: int) -> bool:
    """the superseded fill forms are only in the library `make -C tools/ablation` builds"""
    return variant not in ABLATION_VARIANTS or bool(lib().stb_has_ablation())


def last_error() -> str:
    return lib().stb_last_error().decode()


def check(rc: int) -> None:
    if rc != 0:
        raise StbError(last_error())


class _Resident:
    def __repr__(self):
        return "BPAR_RESIDENT"


BPAR_RESIDENT = _Resident()  # STB_BPAR_RESIDENT: in place of a host bpar, "the concentrations the object holds"


def _bpar(bpar, I: int):
    """the I concentrations of an object call as a host vector (a scalar is broadcast), or the sentinel as it is"""
    if bpar is BPAR_RESIDENT:
        return bpar
    return np.ascontiguousarray(np.broadcast_to(np.asarray(bpar, dtype=np.float64), (I,)))


def dp(a: np.ndarray):
    if a is BPAR_RESIDENT:
        return C.cast(8, c_double_p)
    assert a.dtype == np.float64 and a.flags.c_contiguous
    return a.ctypes.data_as(c_double_p)


# ------------------------------------------------------------------------------------------------
# host interface, mirroring the reference's callers


class Table:
    """`stable_t *` with the reference's accessors as methods (S_make ... S_free)."""

    def __init__(self, initN, initM, maxN, maxM, a, flags=S_STABLE):
        self.L = lib()
        self.sp = self.L.S_make(initN, initM, maxN, maxM, a, flags)
        if not self.sp:
            raise StbError("S_make returned NULL: " + last_error())

    # struct stable_s leading fields (include/stable.h): maxM, maxN, usedM, usedN, startM
    def _u(self, idx):
        return C.cast(self.sp, C.POINTER(C.c_uint))[idx]

    maxM = property(lambda s: s._u(0))
    maxN = property(lambda s: s._u(1))
    usedM = property(lambda s: s._u(2))
    usedN = property(lambda s: s._u(3))
    startM = property(lambda s: s._u(4))

    def remake(self, a):
        return self.L.S_remake(self.sp, a)

    def S(self, n, m):
        return self.L.S_S(self.sp, n, m)

    def S1(self, n):
        return self.L.S_S1(self.sp, n)

    def V(self, n, m):
        return self.L.S_V(self.sp, n, m)

    def U(self, n, m):
        return self.L.S_U(self.sp, n, m)

    def UV(self, n, m):
        return self.L.S_UV(self.sp, n, m)

    def asympt(self, n, m):
        return self.L.S_asympt(self.sp, n, m)

    def sync(self):
        check(self.L.stb_table_sync(self.sp))

    def mirrored(self):
        """(S blocks, V blocks) of 128 rows copied to the host so far"""
        s, v = C.c_uint(), C.c_uint()
        self.L.stb_table_mirrored(self.sp, C.byref(s), C.byref(v))
        return s.value, v.value

    def free(self):
        if self.sp:
            self.L.S_free(self.sp)
            self.sp = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ------------------------------------------------------------------------------------------------
# device interface (torch owns the buffers)


def _torch():
    import torch

    if not torch.cuda.is_available():
        raise StbError("no GPU visible to torch; the device interface has no CPU path")
    return torch


def stream_ptr(stream=None):
    torch = _torch()
    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


class DeviceTables:
    """D log-Stirling tables resident in HBM, filled by one batched call (K1/K2)."""

    def __init__(self, N: int, M: int, D: int = 1, device="cuda"):
        torch = _torch()
        self.L = lib()
        self.N, self.M, self.D = N, M, D
        self.cells = int(self.L.stb_cells(N, M))
        self.elems = int(self.L.stb_elems(N, M))
        self.stride = max(32, (self.elems + 31) // 32 * 32)
        self.tables = torch.empty((D, self.stride), dtype=torch.float64, device=device)
        self.S1 = torch.empty((D, N), dtype=torch.float64, device=device)
        self.ws_bytes = int(self.L.stb_fill_workspace_bytes(N, M, D))
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=device)
        self.a = None

    def fill(self, a, variant=FILL_SCALED, stream=None):
        a = np.ascontiguousarray(np.atleast_1d(np.asarray(a, dtype=np.float64)))
        assert a.shape[0] == self.D
        self.a = a
        check(self.L.stb_fill_S(dp(a), self.D, self.N, self.M, self.tables.data_ptr(), self.stride,
                                self.S1.data_ptr(), self.N, self.ws.data_ptr(), self.ws_bytes,
                                variant, stream_ptr(stream)))

    def status(self):
        """wait for the last fill of this thread and raise if a chain-form fill gave up"""
        check(self.L.stb_fill_status())

    def rowoff(self, n):
        return int(self.L.stb_rowoff(n, self.M))

    def row(self, d, n):
        """values m=2..min(n-1,M) of row n as a device tensor view"""
        ln = min(n - 2, self.M - 1)
        o = self.rowoff(n)
        return self.tables[d, o:o + ln]

    def packed_host(self, d=0):
        """the table without row padding, in the oracle's packed order (numpy)"""
        t = self.tables[d].cpu().numpy()
        N, M = self.N, self.M
        out = np.empty(self.cells, dtype=np.float64)
        pos = 0
        for n in range(3, N + 1):
            ln = min(n - 2, M - 1)
            o = self.rowoff(n)
            out[pos:pos + ln] = t[o:o + ln]
            pos += ln
        return out

    def lookup(self, n, m, d=0, stream=None):
        torch = _torch()
        n = torch.as_tensor(np.asarray(n, dtype=np.uint32).view(np.int32), device=self.tables.device)
        m = torch.as_tensor(np.asarray(m, dtype=np.uint32).view(np.int32), device=self.tables.device)
        out = torch.empty(n.shape[0], dtype=torch.float64, device=self.tables.device)
        check(self.L.stb_lookup_S(self.tables[d].data_ptr(), self.S1[d].data_ptr(), self.N, self.M,
                                  n.data_ptr(), m.data_ptr(), n.shape[0], out.data_ptr(),
                                  stream_ptr(stream)))
        return out.cpu().numpy()


class DeviceSlopeTables:
    """D tables of g = d log S / da and their dS1 vectors (stb_fill_dS); with_S: the log S slabs of the same call too"""

    def __init__(self, N: int, M: int, D: int = 1, device="cuda", with_S: bool = False):
        torch = _torch()
        self.L = lib()
        self.N, self.M, self.D = N, M, D
        self.cells = int(self.L.stb_cells(N, M))
        self.elems = int(self.L.stb_elems(N, M))
        self.stride = max(32, (self.elems + 31) // 32 * 32)
        self.g = torch.full((D, self.stride), float("nan"), dtype=torch.float64, device=device)
        self.dS1 = torch.empty((D, N), dtype=torch.float64, device=device)
        self.tables = torch.empty((D, self.stride), dtype=torch.float64, device=device) if with_S else None
        self.S1 = torch.empty((D, N), dtype=torch.float64, device=device) if with_S else None
        self.ws_bytes = int(self.L.stb_fill_dS_workspace_bytes(N, M, D))
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=device)

    def fill(self, a, stream=None):
        a = np.ascontiguousarray(np.atleast_1d(np.asarray(a, dtype=np.float64)))
        assert a.shape[0] == self.D
        self.a = a
        check(self.L.stb_fill_dS(dp(a), self.D, self.N, self.M, self.g.data_ptr(), self.stride, self.dS1.data_ptr(), self.N,
                                 self.tables.data_ptr() if self.tables is not None else None, self.stride,
                                 self.S1.data_ptr() if self.S1 is not None else None, self.N,
                                 self.ws.data_ptr(), self.ws_bytes, stream_ptr(stream)))

    def packed_host(self, d=0, which="g"):
        """the slab without row padding, in the packed order of the truth (numpy)"""
        t = (self.g if which == "g" else self.tables)[d].cpu().numpy()
        out = np.empty(self.cells, dtype=np.float64)
        pos = 0
        for n in range(3, self.N + 1):
            ln = min(n - 2, self.M - 1)
            o = int(self.L.stb_rowoff(n, self.M))
            out[pos:pos + ln] = t[o:o + ln]
            pos += ln
        return out

    def lookup(self, n, m, d=0, stream=None):
        torch = _torch()
        n = torch.as_tensor(np.asarray(n, dtype=np.uint32).view(np.int32), device=self.g.device)
        m = torch.as_tensor(np.asarray(m, dtype=np.uint32).view(np.int32), device=self.g.device)
        out = torch.empty(n.shape[0], dtype=torch.float64, device=self.g.device)
        check(self.L.stb_lookup_dS(self.g[d].data_ptr(), self.dS1[d].data_ptr(), self.N, self.M, n.data_ptr(), m.data_ptr(),
                                   n.shape[0], out.data_ptr(), stream_ptr(stream)))
        return out.cpu().numpy()


class DeviceFloatTables(DeviceTables):
    """D log-Stirling tables stored as floats (S_FLOAT), written once by the fill that narrows before the store"""

    def __init__(self, N: int, M: int, D: int = 1, device="cuda"):
        super().__init__(N, M, D, device)
        torch = _torch()
        self.tables = torch.empty((D, self.stride), dtype=torch.float32, device=device)

    def fill(self, a, stream=None):
        a = np.ascontiguousarray(np.atleast_1d(np.asarray(a, dtype=np.float64)))
        self.a = a
        check(self.L.stb_fill_Sf(dp(a), self.D, self.N, self.M, self.tables.data_ptr(), self.stride,
                                 self.S1.data_ptr(), self.N, self.ws.data_ptr(), self.ws_bytes, stream_ptr(stream)))

    def packed_host(self, d=0):
        t = self.tables[d].cpu().numpy()
        out = np.empty(self.cells, dtype=np.float32)
        pos = 0
        for n in range(3, self.N + 1):
            ln = min(n - 2, self.M - 1)
            o = self.rowoff(n)
            out[pos:pos + ln] = t[o:o + ln]
            pos += ln
        return out


class DeviceVTables:
    def __init__(self, N: int, M: int, D: int = 1, device="cuda", dtype="f64"):
        torch = _torch()
        self.L = lib()
        self.N, self.M, self.D = N, M, D
        self.cells = int(self.L.stb_vcells(N, M))
        self.elems = int(self.L.stb_velems(N, M))
        self.stride = max(32, (self.elems + 31) // 32 * 32)
        self.dtype = dtype
        self.tables = torch.empty((D, self.stride), dtype=torch.float32 if dtype == "f32" else torch.float64, device=device)
        self.ws_bytes = int(self.L.stb_fill_workspace_bytes(N, M, D))
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=device)

    def fill(self, a, stream=None, exact=False):
        """exact: the reference's own V recurrence, bit for bit (what tables below 512 rows get anyway)"""
        a = np.ascontiguousarray(np.atleast_1d(np.asarray(a, dtype=np.float64)))
        f = self.L.stb_fill_Vf if self.dtype == "f32" else (self.L.stb_fill_V_exact if exact else self.L.stb_fill_V)
        check(f(dp(a), self.D, self.N, self.M, self.tables.data_ptr(), self.stride,
                self.ws.data_ptr(), self.ws_bytes, stream_ptr(stream)))

    def packed_host(self, d=0):
        t = self.tables[d].cpu().numpy()
        out = np.empty(self.cells, dtype=t.dtype)
        pos = 0
        for n in range(2, self.N + 1):
            ln = min(n - 1, self.M - 1)
            o = int(self.L.stb_vrowoff(n, self.M))
            out[pos:pos + ln] = t[o:o + ln]
            pos += ln
        return out


class DeviceGroups:
    """(n,t) pairs and per-restaurant totals resident in HBM (torch tensors)."""

    def __init__(self, g, device="cuda"):
        torch = _torch()
        self.g = g
        self.G = g.pairs
        self.I = g.I
        self.n = torch.as_tensor(g.n.view(np.int32), device=device)
        self.t = torch.as_tensor(g.t.view(np.int16), device=device)
        self.T = torch.as_tensor(g.T.view(np.int32), device=device)
        self.bpar = torch.as_tensor(g.bpar, device=device)


TC_REF_WINDOW = 1  # stb_tcounts_sweep_window / stb_sample_tcounts_window flag: the reference's chain


class _BGroupsMixin:
    """the per-group concentration step on an object (stb_*_set_bpar, _get_bpar, _set_bgroups, _sampleb_groups)"""

    def _hb(self, name):
        return getattr(self.L, "stb_%s_%s" % (self._hb_prefix, name))

    def set_bpar(self, bpar):
        check(self._hb("set_bpar")(self.h, dp(_bpar(bpar, self.I))))

    def get_bpar(self):
        out = np.zeros(self.I, dtype=np.float64)
        check(self._hb("get_bpar")(self.h, dp(out)))
        return out

    def set_bgroups(self, goff=None):
        """contiguous ranges goff[G+1] of restaurants that share a concentration (None: every restaurant its own)"""
        if goff is None:
            check(self._hb("set_bgroups")(self.h, 0, None))
            self.nbgroups = self.I
            return
        goff = np.ascontiguousarray(goff, dtype=np.uint64)
        check(self._hb("set_bgroups")(self.h, int(goff.shape[0]) - 1, goff.ctypes.data_as(C.POINTER(C.c_uint64))))
        self.nbgroups = int(goff.shape[0]) - 1

    def sampleb_groups(self, a, shape, scale, seed: int, sweep: int, want_bgrp: bool = True):
        """one exact step for every group's concentration on the current counts, behind the queued sweeps: (b_g [G] or
        None, BGroupsInfo).  The new concentrations stay on the device: pass BPAR_RESIDENT where a call takes bpar"""
        G = getattr(self, "nbgroups", self.I)
        bgrp = np.zeros(G, dtype=np.float64) if want_bgrp else None
        info = BGroupsInfo()
        rc = self._hb("sampleb_groups")(self.h, float(a), float(shape), float(scale), seed, sweep,
                                        None if bgrp is None else dp(bgrp), C.byref(info))
        if rc:
            err = StbError(last_error())
            err.info = info
            raise err
        return bgrp, info


class TableCounts(_BGroupsMixin):
    """Table counts t of (n, t) pairs resampled on the device by collapsed Gibbs sweeps (stb_tcounts_*).  K, n, t
    (and h, NULL: all 1) in the CSR layout of synth.Groups; M = 0 draws from the full conditional (the largest n)."""

    _hb_prefix = "tcounts"

    def __init__(self, K, n, t, h=None, M: int = 0):
        self.L = lib()
        K = np.ascontiguousarray(K, dtype=np.int32)
        n = np.ascontiguousarray(n, dtype=np.uint32)
        t = np.ascontiguousarray(t, dtype=np.uint16)
        self.I, self.G = int(K.shape[0]), int(n.shape[0])
        hp = None if h is None else dp(np.ascontiguousarray(h, dtype=np.float64))
        self.h = self.L.stb_tcounts_create(self.I, K.ctypes.data_as(c_int_p), n.ctypes.data_as(c_u32_p),
                                           t.ctypes.data_as(c_u16_p), hp, M)
        if not self.h:
            raise StbError(last_error())

    def set_h(self, h=None):
        check(self.L.stb_tcounts_set_h(self.h, None if h is None else dp(np.ascontiguousarray(h, dtype=np.float64))))

    def sweep(self, a, bpar, seed: int, sweep: int, nsweeps: int = 1):
        """sweeps sweep .. sweep+nsweeps-1, queued (bpar: the I concentrations)"""
        bpar = _bpar(bpar, self.I)
        check(self.L.stb_tcounts_sweep(self.h, float(a), dp(bpar), seed, sweep, nsweeps))

    def sweep_window(self, a, bpar, window: int, seed: int, sweep: int, nsweeps: int = 1, ref: bool = False):
        """windowed sweeps sweep .. sweep+nsweeps-1, queued: t moves at most `window` a visit, by an exact
        Metropolis-Hastings step (ref: the reference's chain, every proposal accepted)"""
        bpar = _bpar(bpar, self.I)
        check(self.L.stb_tcounts_sweep_window(self.h, float(a), dp(bpar), int(window), TC_REF_WINDOW if ref else 0, seed,
                                              sweep, nsweeps))

    def get(self):
        """(t[G] uint16, T[I] uint32) after the queued sweeps"""
        t = np.zeros(self.G, dtype=np.uint16)
        T = np.zeros(self.I, dtype=np.uint32)
        check(self.L.stb_tcounts_get(self.h, t.ctypes.data_as(c_u16_p), T.ctypes.data_as(c_u32_p)))
        return t, T

    def to_groups(self, groups, bpar=None):
        """pairs and T to a group set (an stb_groups_create handle) of the same shape, device to device"""
        bp = None if bpar is None else dp(_bpar(bpar, self.I))
        check(self.L.stb_tcounts_to_groups(self.h, groups, bp))

    def sampleb(self, b, shape, scale, a, seed: int, sweep: int, loops: int = 1, verbose: int = 0):
        """one concentration step on the current counts, behind the queued sweeps (stb_tcounts_sampleb): Q is drawn on the
        device from (seed, sweep), b by ARMS / the slice sampler (a > 0) or the Gamma draw (a = 0).  NaN -> StbError"""
        r = float(self.L.stb_tcounts_sampleb(self.h, float(b), float(shape), float(scale), float(a), None, loops, verbose,
                                            seed, sweep))
        if r != r:
            raise StbError(last_error())
        return r

    def samplejoint(self, groups, rect, a, b, shape, scale, seed: int, sweep: int, D: int = 0, J: int = 0,
                    keep_L: bool = False):
        """one joint step for (a, b) on the current counts through the group set `groups`, behind the queued sweeps
        (stb_tcounts_samplejoint); see groups_samplejoint"""
        return _joint_call(self.L.stb_tcounts_samplejoint, (self.h, groups), rect, a, b, shape, scale, seed, sweep, D, J,
                           keep_L)

    def logjoint(self, a, bpar, indicators: bool = False, want_Li: bool = True):
        """(total, L_i[I] or None, LogJointInfo): the log joint probability of the current state, behind the queued sweeps
        (stb_tcounts_logjoint); indicators: the table-indicator representation"""
        bpar = _bpar(bpar, self.I)
        Li = np.zeros(self.I, dtype=np.float64) if want_Li else None
        tot, info = C.c_double(0.0), LogJointInfo()
        check(self.L.stb_tcounts_logjoint(self.h, float(a), dp(bpar), LJ_INDICATORS if indicators else 0, C.byref(tot),
              None if Li is None else dp(Li), C.byref(info)))
        return tot.value, Li, info

    def partition(self, a, hist, bpar, seed: int, sweep: int):
        """stage 1 of the S-free discount step on the current pairs, queued: the table-size histogram into `hist` (a
        Histogram with I restaurants and S > the largest n), with T and bpar (stb_tcounts_partition)"""
        bpar = _bpar(bpar, self.I)
        check(self.L.stb_tcounts_partition(self.h, float(a), hist.h, dp(bpar), seed, sweep))

    def free(self):
        if self.h:
            self.L.stb_tcounts_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def sample_tcounts_window(tabs, a, bpar, koff, n, t, T, h, window: int, seed: int, sweep: int, ref: bool = False,
                          stream=None):
    """one windowed sweep (stb_sample_tcounts_window) on device arrays, t and T in place: tabs a DeviceTables filled for
    `a` (its first slab and its bounds N, M are used), koff (int64 [I+1]), n (int32), t (int16), T (int32), bpar and h
    (float64; h None: all 1) torch tensors on the device"""
    check(lib().stb_sample_tcounts_window(tabs.tables.data_ptr(), tabs.S1.data_ptr(), tabs.N, tabs.M, float(a),
                                          bpar.data_ptr(), int(koff.shape[0]) - 1, koff.data_ptr(), n.data_ptr(),
                                          t.data_ptr(), T.data_ptr(), None if h is None else h.data_ptr(), int(window),
                                          TC_REF_WINDOW if ref else 0, seed, sweep, stream_ptr(stream)))


def logjoint(tabs, a, bpar, koff, n, t, T=None, h=None, indicators: bool = False, want_Li: bool = True, stream=None,
             flags=None):
    """stb_logjoint on device arrays: tabs a DeviceTables filled for `a` (its first slab and its bounds N, M are used), a
    pair (N, M) of bounds alone (no table: no pair may need one), koff (int64 [I+1]), n (int32), t (int16), T (int32, or
    None), bpar and h (float64; h None: all 1) torch tensors on the device.  Returns (total, L_i as a float64 device
    tensor or None, LogJointInfo)."""
    torch = _torch()
    I = int(koff.shape[0]) - 1
    if isinstance(tabs, tuple):
        tp, sp, N, M = None, None, int(tabs[0]), int(tabs[1])
    else:
        tp, sp, N, M = tabs.tables.data_ptr(), tabs.S1.data_ptr(), tabs.N, tabs.M
    Li = torch.empty(max(I, 1), dtype=torch.float64, device=koff.device)[:I] if want_Li else None
    tot, info = C.c_double(0.0), LogJointInfo()
    fl = (LJ_INDICATORS if indicators else 0) if flags is None else int(flags)
    check(lib().stb_logjoint(tp, sp, N, M, float(a), None if bpar is None else bpar.data_ptr(), I, koff.data_ptr(),
                             n.data_ptr(), t.data_ptr(), None if T is None else T.data_ptr(),
                             None if h is None else h.data_ptr(), fl, None if Li is None else Li.data_ptr(), C.byref(tot),
                             C.byref(info), stream_ptr(stream)))
    return tot.value, Li, info


def predict_dishes(a, bpar, koff, n, t, h=None, tstride: int = 0, hoff=None, hcls=None, lik=None, p=None,
                   accumulate: bool = False, skipped=None, stream=None, flags=None):
    """stb_predict_dishes on device arrays: koff (int64 [I+1]), n (int32), t (int16), bpar and h (float64; h None: all 1),
    hoff (int64 [I+1], or None: no held-out customers), hcls (int32 holding uint32 classes), lik (float64 (rows, stride), or
    None: all 1) torch tensors on the device.  tstride > 0: theta comes back as a float64 (I, tstride) device tensor.  p: a
    float64 device tensor of hoff[I] values the call overwrites or (accumulate) adds to; None with hoff: a new one (zeros
    when accumulating).  skipped: None, or an int64 device tensor of one element the call adds to.  Queued, no wait.
    Returns (theta or None, p or None)."""
    torch = _torch()
    I = int(koff.shape[0]) - 1
    theta = torch.empty((max(I, 1), tstride), dtype=torch.float64, device=koff.device)[:I] if tstride > 0 else None
    if hoff is not None and p is None:
        Hc = int(hoff[-1].item())
        p = torch.zeros(max(Hc, 1), dtype=torch.float64, device=koff.device)[:Hc]
    rows, stride = (int(lik.shape[0]), int(lik.shape[1])) if lik is not None else (0, 0)
    fl = (PR_ACCUMULATE if accumulate else 0) if flags is None else int(flags)
    ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    check(lib().stb_predict_dishes(float(a), ptr(bpar), I, koff.data_ptr(), n.data_ptr(), t.data_ptr(), ptr(h), ptr(theta),
                                   int(tstride), ptr(hoff), ptr(hcls), ptr(lik), rows, stride, ptr(p), fl, ptr(skipped),
                                   stream_ptr(stream)))
    return theta, p


def heldout_loglik(p, hoff, samples: int = 1, want_Hi: bool = True, stream=None):
    """stb_heldout_loglik on device tensors p (float64 [hoff[I]]) and hoff (int64 [I+1]): (sum_c log(p_c / samples), H_i as
    a float64 device tensor or None, PredictInfo), after one wait"""
    torch = _torch()
    I = int(hoff.shape[0]) - 1
    Hi = torch.empty(max(I, 1), dtype=torch.float64, device=hoff.device)[:I] if want_Hi else None
    tot, info = C.c_double(0.0), PredictInfo()
    check(lib().stb_heldout_loglik(p.data_ptr(), hoff.data_ptr(), I, int(samples), None if Hi is None else Hi.data_ptr(),
                                   C.byref(tot), C.byref(info), stream_ptr(stream)))
    return tot.value, Hi, info


def seat_customers(a, bpar, koff, n, t, coff, h=None, M: int = 0, cls=None, lik=None, particles: int = 1,
                   commit: bool = False, seed: int = 0, sweep: int = 0, T=None, cust=None, want_p: bool = True, info=None,
                   stream=None, flags=None):
    """stb_seat_customers on device tensors: koff, coff (int64 [I+1]), n (int32 holding uint32), t (int16 holding uint16),
    bpar and h (float64; h None: all 1), cls (int32 holding uint32 classes), lik (float64 (rows, stride), or None: all 1).
    commit: particles must be 1; n and t are written, and T (int32 [I]), cust (int32 [C]) and, with want_p, p (float64 [C])
    are made where not given.  info: None, or an int64 device tensor of three elements the call adds to (skipped,
    impossible, stuck).  Queued, no wait.  Returns (lw float64 (I, particles), T, cust, p), the last three None without
    commit."""
    torch = _torch()
    I = int(koff.shape[0]) - 1
    dev = koff.device
    lw = torch.empty((max(I, 1), max(int(particles), 1)), dtype=torch.float64, device=dev)[:I]
    fl = (SEAT_COMMIT if commit else 0) if flags is None else int(flags)
    p = None
    if fl & SEAT_COMMIT:
        Cc = int(coff[-1].item())
        T = torch.zeros(max(I, 1), dtype=torch.int32, device=dev)[:I] if T is None else T
        cust = torch.zeros(max(Cc, 1), dtype=torch.int32, device=dev)[:Cc] if cust is None else cust
        p = torch.zeros(max(Cc, 1), dtype=torch.float64, device=dev)[:Cc] if want_p else None
    rows, stride = (int(lik.shape[0]), int(lik.shape[1])) if lik is not None else (0, 0)
    ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    check(lib().stb_seat_customers(float(a), ptr(bpar), I, koff.data_ptr(), n.data_ptr(), t.data_ptr(), ptr(T), ptr(h), int(M),
                                   coff.data_ptr(), ptr(cls), ptr(cust), ptr(lik), rows, stride, int(particles), fl, seed,
                                   sweep, lw.data_ptr(), ptr(p), ptr(info), stream_ptr(stream)))
    return lw, T, cust, p


def seat_loglik(lw, want_Hi: bool = True, stream=None):
    """stb_seat_loglik on a device tensor lw (float64 (I, particles)): (sum_i H_i, H_i as a float64 device tensor or None,
    SeatInfo), H_i = log((1/R) sum_r exp(lw_ir)), after one wait"""
    torch = _torch()
    I, R = int(lw.shape[0]), int(lw.shape[1])
    Hi = torch.empty(max(I, 1), dtype=torch.float64, device=lw.device)[:I] if want_Hi else None
    tot, info = C.c_double(0.0), SeatInfo()
    check(lib().stb_seat_loglik(lw.data_ptr(), I, R, None if Hi is None else Hi.data_ptr(), C.byref(tot), C.byref(info),
                                stream_ptr(stream)))
    return tot.value, Hi, info


def seat_filter_budget(K: int) -> int:
    """stb_seat_filter_budget: the largest number of particles stb_seat_filter takes for a restaurant of K dishes"""
    return int(lib().stb_seat_filter_budget(int(K)))


def seat_filter(a, bpar, koff, n, t, coff, h=None, M: int = 0, cls=None, lik=None, particles: int = 1, tau: float = 0.5,
                seed: int = 0, sweep: int = 0, want_w: bool = True, want_states: bool = True, info=None, stream=None, out=None):
    """stb_seat_filter on device tensors (as seat_customers takes them; n and t are read only).  Queued, no wait.  Returns a
    dict of device tensors: Hi float64 [I], and with want_w: w float64 (I, particles), E int64 [I], res int32 (holding
    uint32) [I]; with want_states: pn int32 (holding uint32) and pt int16 (holding uint16), koff[I] * particles each, slot
    r of restaurant i at koff[i] particles + r K_i + k.  info: None, or an int64 device tensor of five elements the call
    adds to (skipped, impossible, stuck, dead, resamplings).  out: a dict of tensors to write into instead of new ones."""
    torch = _torch()
    I = int(koff.shape[0]) - 1
    dev = koff.device
    R = max(int(particles), 1)
    o = dict(out) if out else {}
    if "Hi" not in o:
        o["Hi"] = torch.zeros(max(I, 1), dtype=torch.float64, device=dev)[:I]
    if want_w and "w" not in o:
        o["w"] = torch.zeros((max(I, 1), R), dtype=torch.float64, device=dev)[:I]
        o["E"] = torch.zeros(max(I, 1), dtype=torch.int64, device=dev)[:I]
        o["res"] = torch.zeros(max(I, 1), dtype=torch.int32, device=dev)[:I]
    if want_states and "pn" not in o:
        G = int(koff[-1].item()) * R
        o["pn"] = torch.zeros(max(G, 1), dtype=torch.int32, device=dev)[:G]
        o["pt"] = torch.zeros(max(G, 1), dtype=torch.int16, device=dev)[:G]
    rows, stride = (int(lik.shape[0]), int(lik.shape[1])) if lik is not None else (0, 0)
    ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    check(lib().stb_seat_filter(float(a), ptr(bpar), I, koff.data_ptr(), n.data_ptr(), t.data_ptr(), ptr(h), int(M),
                                coff.data_ptr(), ptr(cls), ptr(lik), rows, stride, int(particles), float(tau), seed, sweep,
                                ptr(o.get("Hi")), ptr(o.get("w")), ptr(o.get("E")), ptr(o.get("res")), ptr(o.get("pn")),
                                ptr(o.get("pt")), ptr(info), stream_ptr(stream)))
    return o


def lik_temper(lik, beta: float, out=None, stream=None):
    """stb_lik_temper on a device tensor lik (float64 (rows, stride)): lik^beta cell by cell (0 stays 0), the matrix the
    dish sweeps of stb_seat_anneal read at temperature beta.  Queued, no wait."""
    torch = _torch()
    out = torch.empty_like(lik) if out is None else out
    check(lib().stb_lik_temper(lik.data_ptr(), int(lik.shape[0]), int(lik.shape[1]), float(beta), out.data_ptr(),
                               stream_ptr(stream)))
    return out


def seat_anneal(tabs, a, bpar, koff, coff, cls, lik, h=None, particles: int = 1, S: int = 1, betas=None, passes: int = 1,
                seed: int = 0, sweep: int = 0, want_states: bool = True, info=None, stream=None, G=None, C_=None,
                bounds=None, ws=None):
    """stb_seat_anneal on device tensors (as seat_customers takes them) for restaurants that start empty.  tabs: a
    DeviceVTables filled for a (None with bounds=(N, M): no table).  betas: None (the even ladder) or S values.  G, C_:
    what the caller states for koff[I] and coff[I] (None: read from the tensors).  Queued, no wait.  Returns a dict of
    device tensors: lw float64 (I, particles), to be finished by seat_loglik; with want_states pn int32 (holding uint32),
    pt int16 (holding uint16) [G particles] and pcust int32 [C particles] in the replicated layout (replica i particles +
    r: pairs from koff[i] particles + r K_i, customers from coff[i] particles + r N_i); ws, the workspace (keep it until
    the stream has run the call).  info: None, or an int64 device tensor of three elements the call adds to (skipped,
    dead, stuck)."""
    torch = _torch()
    I = int(koff.shape[0]) - 1
    dev = koff.device
    R = max(int(particles), 1)
    G = int(koff[-1].item()) if G is None else int(G)
    C_ = int(coff[-1].item()) if C_ is None else int(C_)
    N, M = (tabs.N, tabs.M) if bounds is None else bounds
    rows, stride = int(lik.shape[0]), int(lik.shape[1])
    o = {"lw": torch.zeros((max(I, 1), R), dtype=torch.float64, device=dev)[:I]}
    if want_states:
        o["pn"] = torch.zeros(max(G * R, 1), dtype=torch.int32, device=dev)[:G * R]
        o["pt"] = torch.zeros(max(G * R, 1), dtype=torch.int16, device=dev)[:G * R]
        o["pcust"] = torch.zeros(max(C_ * R, 1), dtype=torch.int32, device=dev)[:C_ * R]
    need = int(lib().stb_seat_anneal_workspace_bytes(I, G, C_, R, rows, stride))
    o["ws"] = torch.empty(max(need, 1), dtype=torch.uint8, device=dev) if ws is None else ws
    bp = None
    if betas is not None:
        betas = np.ascontiguousarray(betas, dtype=np.float64)
        bp = dp(betas)
    ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    check(lib().stb_seat_anneal(None if tabs is None else tabs.tables.data_ptr(), int(N), int(M), float(a), ptr(bpar), I,
                                koff.data_ptr(), ptr(h), coff.data_ptr(), ptr(cls), ptr(lik), rows, stride, G, C_,
                                int(particles), int(S), bp, int(passes), seed, sweep, o["lw"].data_ptr(), ptr(o.get("pn")),
                                ptr(o.get("pt")), ptr(o.get("pcust")), ptr(info), o["ws"].data_ptr(), int(o["ws"].numel()),
                                stream_ptr(stream)))
    return o


def reduce_geometry(which: int, I: int, D: int = 1, J: int = 1, waves: int = 0) -> ReduceGeom:
    """stb_reduce_geometry: what stb_sample_logq (GEOM_LOGQ), stb_joint_terms on a D x J grid (GEOM_JOINT_TERMS) or
    stb_logjoint (GEOM_LOGJOINT) launches for I restaurants on the current device; waves 0: what the call would take now"""
    g = ReduceGeom()
    check(lib().stb_reduce_geometry(int(which), int(I), int(D), int(J), int(waves), C.byref(g)))
    return g


def sample_logq(b, scale, N, seed: int, sweep: int, want_L: bool = True, stream=None, coff=None):
    """stb_sample_logq on a device tensor N (int32 holding uint32 counts): (Q, L) with L a float64 device tensor of
    -log q_i (None when want_L is false).  coff (int64 [I+1] prefix sums of the customers, N None): the objects' route"""
    torch = _torch()
    if coff is not None:
        I = int(coff.shape[0]) - 1
        Lt = torch.empty(I, dtype=torch.float64, device=coff.device) if want_L else None
        Q = C.c_double(0.0)
        check(lib().stb_hq_logq(float(b), float(scale), I, None, coff.data_ptr(), Lt.data_ptr() if want_L and I else None,
                                C.byref(Q), seed, sweep, stream_ptr(stream)))
        return Q.value, Lt
    I = int(N.shape[0])
    Lt = torch.empty(I, dtype=torch.float64, device=N.device) if want_L else None
    Q = C.c_double(0.0)
    check(lib().stb_sample_logq(float(b), float(scale), I, N.data_ptr() if I else None, Lt.data_ptr() if want_L and I else None,
                                C.byref(Q), seed, sweep, stream_ptr(stream)))
    return Q.value, Lt


def sample_bgroups(a, shape, scale, T, bpar, seed: int, sweep: int, N=None, coff=None, goff=None, want_Y: bool = True,
                   want_rate: bool = False, stream=None):
    """stb_sample_bgroups on device tensors: T, N (int32 holding uint32 counts; or coff, int64 [I+1] prefix sums of the
    customers), bpar (float64 [I], overwritten with the new concentrations), goff (int64 [G+1] ranges; None: every
    restaurant its own group).  Returns (bgrp [G], L [I], Y [I] int32 or None, rate [G] or None, BGroupsInfo); want_rate
    goes through the private entry point that also writes every group's 1/scale + sum L"""
    torch = _torch()
    I = int(T.shape[0])
    G = I if goff is None else int(goff.shape[0]) - 1
    dev = bpar.device
    bgrp = torch.empty(G, dtype=torch.float64, device=dev)
    Lt = torch.empty(I, dtype=torch.float64, device=dev)
    Yt = torch.empty(I, dtype=torch.int32, device=dev) if want_Y else None
    rate = torch.empty(G, dtype=torch.float64, device=dev) if want_rate else None
    info = BGroupsInfo()
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    head = (float(a), float(shape), float(scale), I, ptr(N), ptr(coff) if coff is not None else None, ptr(T), G,
            None if goff is None else goff.data_ptr(), ptr(bpar), ptr(bgrp), ptr(Lt), ptr(Yt))
    if want_rate:
        rc = lib().stb_hb_bgroups(*head, ptr(rate), seed, sweep, stream_ptr(stream), C.byref(info), b"stb_sample_bgroups")
    else:
        rc = lib().stb_sample_bgroups(*head, seed, sweep, stream_ptr(stream), C.byref(info))
    if rc:
        err = StbError(last_error())
        err.info = info
        raise err
    return bgrp, Lt, Yt, rate, info


def hgroups_opts(alpha, gamma=1.0, shape=1.0, scale=1.0, flags: int = 0, Kmax: int = 0):
    """(the host vector to keep alive or None, HGroupsOpts): gamma a scalar or Kmax values"""
    keep, gp, g0 = _prior(gamma, Kmax)
    return keep, HGroupsOpts(float(alpha), g0, float(shape), float(scale), gp, int(flags), 0)


def sample_hgroups(koff, t, Kmax: int, root, alpha, gamma, seed: int, sweep: int, goff=None, flags: int = 0, shape=1.0,
                   scale=1.0, want=("hgrp", "c", "m"), stream=None):
    """stb_sample_hgroups on device tensors: koff (int64 [I+1] prefix sums of K_i), t (int16 holding the uint16 table
    counts of the pairs), root (float64 [Kmax], overwritten with r'), goff (int64 [G+1] ranges; None: every restaurant its
    own group).  Returns (h [pairs], dict with whichever of hgrp (float64), c, m (int32 holding uint32) `want` names, each
    (G, Kmax), HGroupsInfo)"""
    torch = _torch()
    I = int(koff.shape[0]) - 1
    G = I if goff is None else int(goff.shape[0]) - 1
    dev = root.device
    h = torch.empty(int(t.shape[0]), dtype=torch.float64, device=dev)
    out = {n: torch.empty((G, Kmax), dtype=torch.float64 if n == "hgrp" else torch.int32, device=dev) for n in want}
    keep, opts = hgroups_opts(alpha, gamma, shape, scale, flags, Kmax)
    info = HGroupsInfo()
    ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
    rc = lib().stb_sample_hgroups(I, ptr(koff), ptr(t), Kmax, G, None if goff is None else goff.data_ptr(), C.byref(opts),
                                  ptr(root), ptr(h), ptr(out.get("hgrp")), ptr(out.get("c")), ptr(out.get("m")), seed, sweep,
                                  stream_ptr(stream), C.byref(info))
    if rc:
        err = StbError(last_error())
        err.info = info
        raise err
    return h, out, info


def htree_opts(levels: int, alpha, gamma=1.0, shape=1.0, scale=1.0, flags: int = 0, Kmax: int = 0):
    """(the host vectors to keep alive, HTreeOpts): alpha one value a level, level 1 first (None: the object's own);
    gamma a scalar or Kmax values"""
    keep, gp, g0 = _prior(gamma, Kmax)
    av = None if alpha is None else np.ascontiguousarray(alpha, dtype=np.float64).reshape(-1)
    if av is not None and av.shape != (levels,):
        raise StbError(f"expected {levels} concentrations, got {av.shape[0]}")
    return (keep, av), HTreeOpts(int(levels), None if av is None else dp(av), g0, float(shape), float(scale), gp, int(flags), 0)


def _ptr_array(ptrs):
    """a C array of pointers (None entries are NULL)"""
    return (C.c_void_p * len(ptrs))(*ptrs)


def sample_htree(koff, t, Kmax: int, G, off, root, hnode, alpha, gamma, seed: int, sweep: int, flags: int = 0, shape=1.0,
                 scale=1.0, want=("c", "m"), stream=None):
    """stb_sample_htree on device tensors: koff, t and root as for sample_hgroups; G the nodes of every level, level 1
    first; off[l] (int64 [G[l]+1]) the ranges of level l + 1; hnode[l] (float64 [G[l], Kmax]) the rows of the levels >= 2,
    overwritten, hnode[0] ignored.  Returns (h [pairs], dict with rows (a list, level 1's made here) and whichever of c, m
    (lists of int32 holding uint32) `want` names, HTreeInfo)"""
    torch = _torch()
    I, L = int(koff.shape[0]) - 1, len(G)
    dev = root.device
    h = torch.empty(int(t.shape[0]), dtype=torch.float64, device=dev)
    rows = [torch.empty((int(G[0]), Kmax), dtype=torch.float64, device=dev)] + list(hnode[1:L])
    out = {n: [torch.empty((int(g), Kmax), dtype=torch.int32, device=dev) for g in G] for n in want}
    out["rows"] = rows
    keep, opts = htree_opts(L, alpha, gamma, shape, scale, flags, Kmax)
    info = HTreeInfo()
    ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
    Gv = (C.c_int * L)(*[int(g) for g in G])
    lists = lambda name: _ptr_array([ptr(x) for x in out[name]]) if name in out else None
    rc = lib().stb_sample_htree(I, ptr(koff), ptr(t), Kmax, Gv, _ptr_array([ptr(o) for o in off]), C.byref(opts), ptr(root),
                                _ptr_array([ptr(r) for r in rows]), ptr(h), lists("c"), lists("m"), seed, sweep,
                                stream_ptr(stream), C.byref(info))
    if rc:
        err = StbError(last_error())
        err.info = info
        raise err
    return h, out, info


def _prior(v, n: int):
    """a Dirichlet parameter, a scalar for every entry or n values, as (the host vector to keep alive or None, its pointer or
    None, the scalar)"""
    if np.ndim(v) == 0:
        return None, None, float(v)
    vec = np.ascontiguousarray(v, dtype=np.float64)
    if vec.shape != (n,):
        raise StbError(f"expected a scalar or {n} values, got shape {vec.shape}")
    return vec, dp(vec), 0.0


def sample_lik(cnt, beta, seed: int, sweep: int, out=None, stream=None):
    """stb_sample_lik on a device tensor cnt (int32 holding uint32 counts, (rows, stride)): a float64 device tensor of the
    same shape whose column k is a draw from Dirichlet(beta_w + cnt[w, k]); beta a scalar or rows values"""
    torch = _torch()
    rows, stride = int(cnt.shape[0]), int(cnt.shape[1])
    lik = torch.empty((rows, stride), dtype=torch.float64, device=cnt.device) if out is None else out
    keep, bp, b0 = _prior(beta, rows)
    check(lib().stb_sample_lik(cnt.data_ptr(), rows, stride, bp, b0, lik.data_ptr(), seed, sweep, stream_ptr(stream)))
    return lik


def sample_classes(lik, cust, seed: int, sweep: int, cls, mask=None, info=None, stream=None):
    """stb_sample_classes on device tensors: lik float64 (rows, stride), cust int32 holding uint32 dishes (C), cls int32
    holding uint32 classes (C; written where a class is drawn), mask uint8 (C) or None, info int64 (3: skipped, stuck,
    drawn, added to) or None.  Returns cls"""
    rows, stride = int(lik.shape[0]), int(lik.shape[1])
    check(lib().stb_sample_classes(lik.data_ptr(), rows, stride, cust.data_ptr(), None if mask is None else mask.data_ptr(),
                                   int(cust.shape[0]), seed, sweep, cls.data_ptr(), None if info is None else info.data_ptr(),
                                   stream_ptr(stream)))
    return cls


def lik_loglik(cnt, lik, stream=None):
    """stb_lik_loglik on device tensors cnt (int32 holding uint32) and lik (float64), both (rows, stride):
    (sum cnt log lik, cells with a count and no likelihood)"""
    rows, stride = int(cnt.shape[0]), int(cnt.shape[1])
    tot, imp = C.c_double(0.0), C.c_uint64(0)
    check(lib().stb_lik_loglik(cnt.data_ptr(), lik.data_ptr(), rows, stride, C.byref(tot), C.byref(imp), stream_ptr(stream)))
    return tot.value, imp.value


def gauss_prior(kappa0, alpha0, beta0, m0=None, D: int = 0):
    """(a GaussPrior, what keeps its vectors alive): beta0 a scalar or D values, m0 None (zeros) or D values"""
    keep = []
    p = GaussPrior(float(kappa0), float(alpha0), 0.0, None, None)
    if np.ndim(beta0) == 0:
        p.beta00 = float(beta0)
    else:
        keep.append(np.ascontiguousarray(beta0, dtype=np.float64))
        p.beta0 = dp(keep[-1])
    if m0 is not None:
        keep.append(np.ascontiguousarray(m0, dtype=np.float64))
        p.m0 = dp(keep[-1])
    for v in keep:
        if D and v.shape != (D,):
            raise StbError(f"expected a scalar or {D} values, got shape {v.shape}")
    return p, keep


def gauss_stats(x, cust, K: int, out=None, stream=None):
    """stb_gauss_stats on device tensors x float64 (C, D) and cust int32 holding uint32 dishes (C): (n int32 (K), mean
    float64 (K, D), Q float64 (K, D), GaussInfo); out: (n, mean, Q) to write into"""
    torch = _torch()
    Cn, D = int(x.shape[0]), int(x.shape[1])
    if out is None:
        out = (torch.empty(K, dtype=torch.int32, device=x.device), torch.empty((K, D), dtype=torch.float64, device=x.device),
               torch.empty((K, D), dtype=torch.float64, device=x.device))
    n, mean, Q = out
    info = GaussInfo()
    check(lib().stb_gauss_stats(x.data_ptr(), D, cust.data_ptr(), Cn, K, n.data_ptr(), mean.data_ptr(), Q.data_ptr(),
                                C.byref(info), stream_ptr(stream)))
    return n, mean, Q, info


def sample_gauss(n, mean, Q, prior, seed: int, sweep: int, stream=None):
    """stb_sample_gauss on the statistics of gauss_stats: (mu, tau), float64 device tensors (K, D); prior a GaussPrior (or
    the pair gauss_prior returns)"""
    torch = _torch()
    K, D = int(mean.shape[0]), int(mean.shape[1])
    p = prior[0] if isinstance(prior, tuple) else prior
    mu, tau = torch.empty_like(mean), torch.empty_like(mean)
    check(lib().stb_sample_gauss(n.data_ptr(), mean.data_ptr(), Q.data_ptr(), K, D, C.byref(p), seed, sweep, mu.data_ptr(),
                                 tau.data_ptr(), stream_ptr(stream)))
    return mu, tau


def gauss_lik(x, mu, tau, stride: int = 0, out=None, stream=None):
    """stb_gauss_lik: the (C, stride) matrix exp(l_ck - max_k l_ck) of the Gaussian densities (stride = 0: K), and GaussInfo"""
    torch = _torch()
    Cn, D, K = int(x.shape[0]), int(x.shape[1]), int(mu.shape[0])
    stride = int(stride) if stride else K
    lik = torch.empty((Cn, stride), dtype=torch.float64, device=x.device) if out is None else out
    info = GaussInfo()
    check(lib().stb_gauss_lik(x.data_ptr(), D, Cn, mu.data_ptr(), tau.data_ptr(), K, lik.data_ptr(), stride, C.byref(info),
                              stream_ptr(stream)))
    return lik, info


def gauss_loglik(x, cust, mu, tau, stream=None):
    """stb_gauss_loglik: (log p(x | z, mu, tau), GaussInfo)"""
    Cn, D, K = int(x.shape[0]), int(x.shape[1]), int(mu.shape[0])
    tot, info = C.c_double(0.0), GaussInfo()
    check(lib().stb_gauss_loglik(x.data_ptr(), D, cust.data_ptr(), Cn, mu.data_ptr(), tau.data_ptr(), K, C.byref(tot),
                                 C.byref(info), stream_ptr(stream)))
    return tot.value, info


def gauss_logml(n, mean, Q, prior, stream=None):
    """stb_gauss_logml: the collapsed evidence log p(x | z) from the statistics of gauss_stats"""
    K, D = int(mean.shape[0]), int(mean.shape[1])
    p = prior[0] if isinstance(prior, tuple) else prior
    tot = C.c_double(0.0)
    check(lib().stb_gauss_logml(n.data_ptr(), mean.data_ptr(), Q.data_ptr(), K, D, C.byref(p), C.byref(tot), stream_ptr(stream)))
    return tot.value


def gauss_heldout(theta, hoff, y, mu, tau, want_ell: bool = True, rstride: int = 0, acc=None, stream=None, flags=None):
    """stb_gauss_heldout on device tensors: theta float64 (I, tstride) as predict_dishes returns it, hoff int64 (I + 1), y
    float64 (C_h, D), mu and tau float64 (K, D).  rstride > 0: the responsibilities come back as a float64 (C_h, rstride)
    device tensor.  acc: None, or the pair (M, A) of float64 device tensors (C_h) the call updates (empty: -inf and 0).
    Queued, no wait.  Returns (ell or None, resp or None)."""
    torch = _torch()
    I, Ch, D, K = int(hoff.shape[0]) - 1, int(y.shape[0]), int(y.shape[1]), int(mu.shape[0])
    ell = torch.empty(max(Ch, 1), dtype=torch.float64, device=y.device)[:Ch] if want_ell else None
    resp = torch.empty((max(Ch, 1), rstride), dtype=torch.float64, device=y.device)[:Ch] if rstride > 0 else None
    fl = (GH_ACCUMULATE if acc is not None else 0) if flags is None else int(flags)
    M, A = acc if acc is not None else (None, None)
    ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    check(lib().stb_gauss_heldout(theta.data_ptr(), int(theta.shape[1]), I, hoff.data_ptr(), y.data_ptr(), D, mu.data_ptr(),
                                  tau.data_ptr(), K, ptr(ell), ptr(resp), int(rstride), ptr(M), ptr(A), fl, stream_ptr(stream)))
    return ell, resp


def gauss_heldout_loglik(hoff, ell=None, acc=None, samples: int = 1, want_Hi: bool = True, stream=None):
    """stb_gauss_heldout_loglik: the sum of ell (float64 device tensor), or with acc = (M, A) of sum_j M_j + log(A_j /
    samples): (total, H_i as a float64 device tensor or None, PredictInfo), after one wait"""
    torch = _torch()
    I = int(hoff.shape[0]) - 1
    Hi = torch.empty(max(I, 1), dtype=torch.float64, device=hoff.device)[:I] if want_Hi else None
    tot, info = C.c_double(0.0), PredictInfo()
    M, A = acc if acc is not None else (None, None)
    ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    check(lib().stb_gauss_heldout_loglik(ptr(ell), ptr(M), ptr(A), int(samples), hoff.data_ptr(), I, ptr(Hi), C.byref(tot),
                                         C.byref(info), stream_ptr(stream)))
    return tot.value, Hi, info


def dirmult_logml(cnt, w, orientation: int = DM_ROWS, cols: int = 0, scale=1.0, want_each: bool = True, stream=None):
    """stb_dirmult_logml on a device tensor cnt (int32 holding uint32 counts, (rows, stride); cols = 0: stride columns):
    the log marginal of its rows (DM_ROWS) or columns (DM_COLUMNS) as multinomials under a Dirichlet prior.  w: a float64
    device tensor of weights (one per column / per row) or a scalar for all of them; scale: a float, or a float64 device
    tensor of one element.  Returns (total, one value per multinomial as a device tensor or None, DirMultInfo); a call that
    fails raises StbError with .info set"""
    torch = _torch()
    rows, stride = int(cnt.shape[0]), int(cnt.shape[1])
    cols = int(cols) if cols else stride
    n_each = rows if orientation == DM_ROWS else cols
    each = torch.empty(max(n_each, 1), dtype=torch.float64, device=cnt.device) if want_each else None
    wvec = None if np.ndim(w) == 0 and not hasattr(w, "data_ptr") else w
    svec = scale if hasattr(scale, "data_ptr") else None
    tot, info = C.c_double(0.0), DirMultInfo()
    rc = lib().stb_dirmult_logml(cnt.data_ptr(), rows, cols, stride, int(orientation),
                                 None if wvec is None else wvec.data_ptr(), 0.0 if wvec is not None else float(w),
                                 0.0 if svec is not None else float(scale), None if svec is None else svec.data_ptr(),
                                 None if each is None else each.data_ptr(), C.byref(tot), C.byref(info), stream_ptr(stream))
    if rc:
        err = StbError(last_error())
        err.info = info
        raise err
    return tot.value, (None if each is None else each[:n_each]), info


def sample_dirconc(cnt, v, s, shape, scale, seed: int, sweep: int, orientation: int = DM_ROWS, cols: int = 0,
                   want=("m", "M"), stream=None):
    """stb_sample_dirconc on a device tensor cnt (int32 holding uint32 counts, (rows, stride); cols = 0: stride columns):
    one exact Gibbs step of the scale s of the Dirichlet weights s * v its rows (DM_ROWS) or columns (DM_COLUMNS) share
    as multinomials, under the prior Gamma(shape, scale).  v: a float64 device tensor (one value per column / per row) or
    a scalar for all.  Returns (s', dict with whichever of m ((rows, stride)) and M (one per multinomial) `want` names,
    int32 holding uint32, DirConcInfo); a call that fails raises StbError with .info set"""
    torch = _torch()
    rows, stride = int(cnt.shape[0]), int(cnt.shape[1])
    cols = int(cols) if cols else stride
    nm = rows if orientation == DM_ROWS else cols
    out = {}
    if "m" in want:
        out["m"] = torch.empty((rows, stride), dtype=torch.int32, device=cnt.device)
    if "M" in want:
        out["M"] = torch.empty(max(nm, 1), dtype=torch.int32, device=cnt.device)[:nm]
    vvec = None if np.ndim(v) == 0 and not hasattr(v, "data_ptr") else v
    ncat = cols if orientation == DM_ROWS else rows
    if vvec is not None and (vvec.dtype != torch.float64 or vvec.numel() != ncat):
        raise StbError(f"sample_dirconc: v must be a scalar or {ncat} float64 values on the device")
    info = DirConcInfo()
    ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
    rc = lib().stb_sample_dirconc(ptr(cnt), rows, cols, stride, int(orientation), None if vvec is None else vvec.data_ptr(),
                                  0.0 if vvec is not None else float(v), float(s), float(shape), float(scale), ptr(out.get("m")),
                                  ptr(out.get("M")), seed, sweep, stream_ptr(stream), C.byref(info))
    if rc:
        err = StbError(last_error())
        err.info = info
        raise err
    return info.s, out, info


def sampleb_device(b, shape, scale, N, T, a, seed: int, sweep: int, loops: int = 1, verbose: int = 0, stream=None):
    """stb_sampleb_device on device tensors N, T (int32 holding uint32 counts).  NaN -> StbError"""
    r = float(lib().stb_sampleb_device(float(b), int(N.shape[0]), float(shape), float(scale), N.data_ptr(), T.data_ptr(),
                                       float(a), None, loops, verbose, seed, sweep, stream_ptr(stream)))
    if r != r:
        raise StbError(last_error())
    return r


def groups_samplea(groups, a, loops: int = 1, verbose: int = 0):
    """stb_groups_samplea on a group-set handle (stb_groups_create): the new discount.  NaN -> StbError"""
    r = float(lib().stb_groups_samplea(groups, float(a), None, loops, verbose))
    if r != r:
        raise StbError(last_error())
    return r


def groups_ssum(groups, x):
    """stb_groups_ssum on a group-set handle: W(x_d), the pair sum without the restaurant terms"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.zeros(x.shape[0], dtype=np.float64)
    check(lib().stb_groups_ssum(groups, dp(x), int(x.shape[0]), dp(out)))
    return out


def groups_aterms_grad(groups, x):
    """stb_groups_aterms_grad on a group-set handle: (aterms(x_d), d aterms / dx at x_d)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    val = np.zeros(x.shape[0], dtype=np.float64)
    grad = np.zeros(x.shape[0], dtype=np.float64)
    check(lib().stb_groups_aterms_grad(groups, dp(x), int(x.shape[0]), dp(val), dp(grad)))
    return val, grad


def groups_modea(groups, a_lo, a_hi, tol=1e-9, rounds_max=32):
    """stb_groups_modea on a group-set handle: (a_hat, curvature, ModeaInfo)"""
    a_hat, curv, info = C.c_double(float("nan")), C.c_double(float("nan")), ModeaInfo()
    check(lib().stb_groups_modea(groups, float(a_lo), float(a_hi), float(tol), int(rounds_max), C.byref(a_hat), C.byref(curv),
                                 C.byref(info)))
    return a_hat.value, curv.value, info


def joint_terms(a, b, T, N, stream=None, coff=None):
    """stb_joint_terms on device tensors T, N (int32 holding uint32 counts): R[d, j] as a float64 device tensor.
    coff (int64 [I+1] prefix sums of the customers, N None): the objects' route"""
    torch = _torch()
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    I = int(T.shape[0])
    out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float64, device=T.device)
    if coff is not None:
        check(lib().stb_hj_joint_terms(dp(a), int(a.shape[0]), dp(b), int(b.shape[0]), T.data_ptr(), None, coff.data_ptr(), I,
                                       out.data_ptr(), stream_ptr(stream)))
        return out
    check(lib().stb_joint_terms(dp(a), int(a.shape[0]), dp(b), int(b.shape[0]), T.data_ptr() if I else None,
                                N.data_ptr() if I else None, I, out.data_ptr(), stream_ptr(stream)))
    return out


def _joint_call(fn, head, rect, a, b, shape, scale, seed, sweep, D, J, keep_L):
    o = JointOpts(float(rect[0]), float(rect[1]), float(rect[2]), float(rect[3]), int(D), int(J), float(shape),
                  float(scale), int(seed), int(sweep), JOINT_KEEP_L if keep_L else 0)
    info = JointInfo()
    ao, bo = C.c_double(float(a)), C.c_double(float(b))
    check(fn(*head, C.byref(o), float(a), float(b), C.byref(ao), C.byref(bo), C.byref(info)))
    res = {"a": ao.value, "b": bo.value, "stages": info.stages, "accepted": bool(info.accepted), "evals": info.evals,
           "stage_pick": info.stage_pick, "log_alpha": info.log_alpha, "rect": tuple(info.rect),
           "a_prop": info.a_prop, "b_prop": info.b_prop, "L_cur": info.L_cur, "L_prop": info.L_prop,
           "cell": [info.cell[s] for s in range(info.stages)],
           "box": [tuple(info.box[s]) for s in range(info.stages)]}
    if keep_L:
        DJ = (int(D) or 24) * (int(J) or 24)
        res["L"] = np.ctypeslib.as_array(info.L, shape=(info.stages * DJ,)).reshape(info.stages, DJ).copy()
    return res


def groups_samplejoint(groups, N, rect, a, b, shape, scale, seed: int, sweep: int, D: int = 0, J: int = 0,
                       keep_L: bool = False):
    """stb_groups_samplejoint on a group-set handle and a device tensor N (int32 holding uint32 counts); rect =
    (a_lo, a_hi, b_lo, b_hi).  A dict with the new a, b and the step's diagnostics"""
    return _joint_call(lib().stb_groups_samplejoint, (groups, None if N is None else N.data_ptr()), rect, a, b, shape,
                       scale, seed, sweep, D, J, keep_L)


def sampler_trace():
    """the (x, y) evaluations of this process's most recent sampler call, and ARMS' return code"""
    L = lib()
    xs, ys = [], []
    x, y = C.c_double(), C.c_double()
    for k in range(L.stb_sampler_trace_count()):
        L.stb_sampler_trace_get(k, C.byref(x), C.byref(y))
        xs.append(x.value)
        ys.append(y.value)
    return np.array(xs), np.array(ys), int(L.stb_sampler_trace_code())


PT_REF_WALK = 1  # stb_sample_partition flag: lib/samplea.c's walk, as the drop-in samplea2


class Histogram:
    """A table-size histogram on the device (stb_hist_t): cnt[S] (cnt[s], s >= 2, tables of s customers; cnt[1]
    singletons; cnt[0] pairs left out) with the I restaurants' T and bpar, as aterms2 reads it.  From host counts
    (stb_hist_create) or empty, for a partition call to fill (stb_hist_create_empty)."""

    def __init__(self, S: int, I: int, cnt=None, T=None, bpar=None):
        self.L = lib()
        self.S, self.I = int(S), int(I)
        if cnt is None:
            self.h = self.L.stb_hist_create_empty(self.S, self.I)
        else:
            cnt = np.ascontiguousarray(cnt, dtype=np.uint32)
            T = np.ascontiguousarray(T, dtype=np.uint32)
            bpar = np.ascontiguousarray(bpar, dtype=np.float64)
            assert cnt.shape[0] == self.S and T.shape[0] == self.I and bpar.shape[0] == self.I
            self.h = self.L.stb_hist_create(cnt.ctypes.data_as(c_u32_p), self.S, self.I, T.ctypes.data_as(c_u32_p), dp(bpar))
        if not self.h:
            raise StbError(last_error())

    def restaurants(self, T, bpar):
        T = np.ascontiguousarray(T, dtype=np.uint32)
        bpar = np.ascontiguousarray(np.broadcast_to(np.asarray(bpar, dtype=np.float64), (self.I,)))
        check(self.L.stb_hist_restaurants(self.h, T.ctypes.data_as(c_u32_p), dp(bpar)))

    def device_counts(self):
        """(device address of cnt[S], the histogram's stream as an int)"""
        S, st = C.c_uint(0), C.c_void_p()
        p = self.L.stb_hist_counts_device(self.h, C.byref(S), C.byref(st))
        if not p:
            raise StbError(last_error())
        return p, st.value

    def counts(self):
        """cnt[S] uint32, after the work queued on the histogram"""
        out = np.zeros(self.S, dtype=np.uint32)
        check(self.L.stb_hist_get(self.h, out.ctypes.data_as(c_u32_p)))
        return out

    def aterms2(self, xs):
        """aterms2 at the discounts xs (at most 64 a call; stb_hist_aterms2)"""
        xs = np.ascontiguousarray(np.atleast_1d(np.asarray(xs, dtype=np.float64)))
        out = np.zeros(xs.shape[0])
        check(self.L.stb_hist_aterms2(self.h, dp(xs), int(xs.shape[0]), dp(out)))
        return out

    def free(self):
        if self.h:
            self.L.stb_hist_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def sample_partition(tabs, a, n, t, S: int, seed: int, sweep: int, sizes=None, soff=None, ref: bool = False, cnt=None,
                     stream=None):
    """one partition draw (stb_sample_partition) on device arrays: tabs a DeviceTables filled for `a` (its first slab
    and its bounds N, M), n (int32) and t (int16) torch tensors on the device; sizes (int16) and soff (int64 [G+1]) both
    or neither.  Returns cnt (int32 [S] torch tensor on the device, zeroed and filled on `stream`)."""
    torch = _torch()
    if cnt is None:
        cnt = torch.empty(S, dtype=torch.int32, device=n.device)
    check(lib().stb_sample_partition(tabs.tables.data_ptr(), tabs.S1.data_ptr(), tabs.N, tabs.M, float(a),
                                     int(n.shape[0]), n.data_ptr(), t.data_ptr(), cnt.data_ptr(), int(S),
                                     None if sizes is None else sizes.data_ptr(), None if soff is None else soff.data_ptr(),
                                     PT_REF_WALK if ref else 0, seed, sweep, stream_ptr(stream)))
    return cnt


TD_MAXK = 1024  # STB_TD_MAXK: dishes a restaurant may have under stb_tindic_sweep_dishes / stb_sample_tdishes
TI_REF_ODDS = 1  # stb_tindic_create / stb_sample_tindic flag: the reference's factor t / (n-t+1)


class TableIndicators(_BGroupsMixin):
    """Table counts t of (n, t) pairs resampled on the device customer by customer with table indicators
    (stb_tindic_*).  K, n, t, h as for TableCounts; cust: the customers of every restaurant as local pair indices, back to
    back (None: pair order); M = 0 truncates at the largest n; flags TI_REF_ODDS."""

    _hb_prefix = "tindic"

    def __init__(self, K, n, t, h=None, cust=None, M: int = 0, flags: int = 0):
        self.L = lib()
        K = np.ascontiguousarray(K, dtype=np.int32)
        n = np.ascontiguousarray(n, dtype=np.uint32)
        t = np.ascontiguousarray(t, dtype=np.uint16)
        self.I, self.G = int(K.shape[0]), int(n.shape[0])
        self.h = None
        self.maxK = int(K.max()) if self.I else 0
        if int(K.astype(np.int64).sum()) != self.G or t.shape[0] != self.G or (h is not None and len(h) != self.G):
            raise StbError(f"TableIndicators: sum K = {int(K.astype(np.int64).sum())}, but {self.G} n, {t.shape[0]} t"
                           + ("" if h is None else f", {len(h)} h"))
        C_ = int(n.astype(np.int64).sum())
        cp = None
        if cust is not None:
            cust = np.ascontiguousarray(cust, dtype=np.uint32)
            if cust.shape[0] != C_:
                raise StbError(f"TableIndicators: {cust.shape[0]} customers in cust, sum n = {C_}")
            cp = cust.ctypes.data_as(c_u32_p)
        self.C = C_
        hp = None if h is None else dp(np.ascontiguousarray(h, dtype=np.float64))
        self.h = self.L.stb_tindic_create(self.I, K.ctypes.data_as(c_int_p), n.ctypes.data_as(c_u32_p),
                                          t.ctypes.data_as(c_u16_p), hp, cp, M, flags)
        if not self.h:
            raise StbError(last_error())

    def set_h(self, h=None):
        check(self.L.stb_tindic_set_h(self.h, None if h is None else dp(np.ascontiguousarray(h, dtype=np.float64))))

    def sweep(self, a, bpar, seed: int, sweep: int, nsweeps: int = 1):
        """sweeps sweep .. sweep+nsweeps-1, queued (bpar: the I concentrations)"""
        bpar = _bpar(bpar, self.I)
        check(self.L.stb_tindic_sweep(self.h, float(a), dp(bpar), seed, sweep, nsweeps))

    def get(self):
        """(t[G] uint16, T[I] uint32) after the queued sweeps"""
        t = np.zeros(self.G, dtype=np.uint16)
        T = np.zeros(self.I, dtype=np.uint32)
        check(self.L.stb_tindic_get(self.h, t.ctypes.data_as(c_u16_p), T.ctypes.data_as(c_u32_p)))
        return t, T

    def to_groups(self, groups, bpar=None):
        """pairs and T to a group set (an stb_groups_create handle) of the same shape, device to device"""
        bp = None if bpar is None else dp(_bpar(bpar, self.I))
        check(self.L.stb_tindic_to_groups(self.h, groups, bp))

    def sampleb(self, b, shape, scale, a, seed: int, sweep: int, loops: int = 1, verbose: int = 0):
        """one concentration step on the current counts, behind the queued sweeps (stb_tindic_sampleb): Q is drawn on the
        device from (seed, sweep), b by ARMS / the slice sampler (a > 0) or the Gamma draw (a = 0).  NaN -> StbError"""
        r = float(self.L.stb_tindic_sampleb(self.h, float(b), float(shape), float(scale), float(a), None, loops, verbose,
                                            seed, sweep))
        if r != r:
            raise StbError(last_error())
        return r

    def samplejoint(self, groups, rect, a, b, shape, scale, seed: int, sweep: int, D: int = 0, J: int = 0,
                    keep_L: bool = False):
        """one joint step for (a, b) on the current counts through the group set `groups`, behind the queued sweeps
        (stb_tindic_samplejoint); see groups_samplejoint"""
        return _joint_call(self.L.stb_tindic_samplejoint, (self.h, groups), rect, a, b, shape, scale, seed, sweep, D, J,
                           keep_L)

    def logjoint(self, a, bpar, indicators: bool = False, want_Li: bool = True):
        """(total, L_i[I] or None, LogJointInfo): the log joint probability of the current state, behind the queued sweeps
        (stb_tindic_logjoint); indicators: the table-indicator representation"""
        bpar = _bpar(bpar, self.I)
        Li = np.zeros(self.I, dtype=np.float64) if want_Li else None
        tot, info = C.c_double(0.0), LogJointInfo()
        check(self.L.stb_tindic_logjoint(self.h, float(a), dp(bpar), LJ_INDICATORS if indicators else 0, C.byref(tot),
              None if Li is None else dp(Li), C.byref(info)))
        return tot.value, Li, info

    def logjoint_collapsed(self, a, bpar, alpha=0.0, gamma=1.0, beta=1.0, flags: int = 0):
        """(total, CJInfo): the log joint of the current state with the groups' base weights (and, with CJ_DATA, the dishes'
        class distributions) summed out, behind the queued sweeps (stb_tindic_logjoint_collapsed).  alpha = 0: the
        concentration the last sample_hgroups left; gamma (CJ_FLAT, CJ_ROOT) a scalar or one value per dish; beta (CJ_DATA) a
        scalar or one value per row of the matrix"""
        bpar = _bpar(bpar, self.I)
        keep_g, gp, g0 = _prior(gamma, self.maxK)
        keep_b, bp, b0 = _prior(beta, self.lik_device()[1]) if np.ndim(beta) else (None, None, float(beta))
        opts = CJOpts(float(alpha), g0, b0, gp, bp)
        tot, info = C.c_double(0.0), CJInfo()
        check(self.L.stb_tindic_logjoint_collapsed(self.h, float(a), dp(bpar), int(flags), C.byref(opts), C.byref(tot),
                                                   C.byref(info)))
        return tot.value, info

    # ---- dishes: customers move between the pairs of their restaurant (stb_tindic_sweep_dishes)

    def set_classes(self, cls, rows: int):
        """cls[C]: every customer's likelihood class, < rows (None: none)"""
        if cls is None:
            check(self.L.stb_tindic_set_classes(self.h, None, 0))
            self.rows = 0
            return
        cls = np.ascontiguousarray(cls, dtype=np.uint32)
        if cls.shape[0] != self.C:
            raise StbError(f"TableIndicators.set_classes: {cls.shape[0]} classes, {self.C} customers")
        check(self.L.stb_tindic_set_classes(self.h, cls.ctypes.data_as(c_u32_p), rows))
        self.rows = int(rows)

    def set_lik(self, lik=None, rows: int = 0, stride: int = 0):
        """lik: a (rows, stride) matrix of likelihoods, finite and >= 0, stride >= the largest K; None with rows = 0
        removes it, None with a shape holds all ones (for device writers: lik_device)"""
        if lik is None:
            check(self.L.stb_tindic_set_lik(self.h, None, rows, stride))
        else:
            lik = np.ascontiguousarray(lik, dtype=np.float64)
            if lik.ndim != 2:
                raise StbError("TableIndicators.set_lik: lik must be a (rows, stride) matrix")
            rows, stride = lik.shape
            check(self.L.stb_tindic_set_lik(self.h, dp(lik), rows, stride))
        self.stride = int(stride) if rows else 0

    def lik_device(self):
        """(device pointer or None, rows, stride, stream) of the likelihood matrix"""
        r, st, q = C.c_uint(0), C.c_uint(0), C.c_void_p(None)
        p = self.L.stb_tindic_lik_device(self.h, C.byref(r), C.byref(st), C.byref(q))
        return p, r.value, st.value, q.value

    def sweep_dishes(self, a, bpar, seed: int, sweep: int, nsweeps: int = 1):
        """dish sweeps sweep .. sweep+nsweeps-1; returns TDishInfo (skipped, stuck) of the call, after a wait"""
        bpar = _bpar(bpar, self.I)
        info = TDishInfo()
        check(self.L.stb_tindic_sweep_dishes(self.h, float(a), dp(bpar), seed, sweep, nsweeps, C.byref(info)))
        return info

    def get_state(self):
        """(n[G] uint32, cust[C] uint32) after the queued sweeps"""
        n = np.zeros(self.G, dtype=np.uint32)
        cust = np.zeros(self.C, dtype=np.uint32)
        check(self.L.stb_tindic_get_state(self.h, n.ctypes.data_as(c_u32_p), cust.ctypes.data_as(c_u32_p)))
        return n, cust

    def class_counts(self):
        """customers per (class, dish): uint32 (rows, stride), stride the likelihood's or the largest K"""
        stride = getattr(self, "stride", 0) or max(self.maxK, 1)
        cnt = np.zeros((getattr(self, "rows", 0), stride), dtype=np.uint32)
        if cnt.size == 0:
            raise StbError("TableIndicators.class_counts: classes are not set")
        check(self.L.stb_tindic_class_counts(self.h, cnt.ctypes.data_as(c_u32_p)))
        return cnt

    # ---- the likelihood and the base weights drawn on the device (stb_tindic_sample_lik / _sample_h / _loglik)

    def sample_lik(self, beta, seed: int, sweep: int):
        """the matrix drawn again: column k from Dirichlet(beta_w + customers of class w at dish k), behind the queued
        sweeps; beta a scalar or one value per row of the matrix.  Classes and a matrix must be set"""
        keep, bp, b0 = _prior(beta, self.lik_device()[1])
        check(self.L.stb_tindic_sample_lik(self.h, bp, b0, seed, sweep))

    def sample_h(self, gamma, seed: int, sweep: int):
        """the base weights drawn again: h from Dirichlet(gamma_k + tables of dish k), the same for every restaurant;
        gamma a scalar or one value per dish (the largest K).  Give it another seed than sample_lik"""
        keep, gp, g0 = _prior(gamma, self.maxK)
        check(self.L.stb_tindic_sample_h(self.h, gp, g0, seed, sweep))

    def _sample_conc(self, fn, base, n, s, shape, scale, seed, sweep):
        keep, bp, _ = _prior(base, n) if base is not None and np.ndim(base) else (None, None, 1.0)
        info = DirConcInfo()
        rc = fn(self.h, bp, float(s), float(shape), float(scale), seed, sweep, C.byref(info))
        if rc:
            err = StbError(last_error())
            err.info = info
            raise err
        return info

    def sample_beta(self, s, shape, scale, seed: int, sweep: int, base=None):
        """one exact Gibbs step of the scale of the class distributions' prior beta_w = s * base_w (base: one value per
        row of the matrix, None: 1 each) under s ~ Gamma(shape, scale), from the (class, dish) counts, behind the queued
        sweeps (stb_tindic_sample_beta).  Writes nothing of the state; returns DirConcInfo, .s the new scale"""
        n = self.lik_device()[1] if base is not None and np.ndim(base) else 0
        return self._sample_conc(self.L.stb_tindic_sample_beta, base, n, s, shape, scale, seed, sweep)

    def sample_gamma(self, s, shape, scale, seed: int, sweep: int, base=None):
        """the same for the flat base weights' prior gamma_k = s * base_k (base: one value per dish, None: 1 each), from
        the tables of every dish over all restaurants (stb_tindic_sample_gamma)"""
        return self._sample_conc(self.L.stb_tindic_sample_gamma, base, self.maxK, s, shape, scale, seed, sweep)

    # ---- base weights per group of restaurants under a shared root (stb_tindic_set_hgroups / _set_hroot / _sample_hgroups)

    def set_hgroups(self, goff=None):
        """the contiguous ranges of restaurants that share base weights: goff[G+1] (None: every restaurant its own group)"""
        if goff is None:
            check(self.L.stb_tindic_set_hgroups(self.h, 0, None))
            return
        goff = np.ascontiguousarray(goff, dtype=np.uint64)
        check(self.L.stb_tindic_set_hgroups(self.h, int(goff.shape[0]) - 1, goff.ctypes.data_as(C.POINTER(C.c_uint64))))

    def set_hroot(self, root=None):
        """the root of the groups' base weights: the largest K positive values (None: equal weights)"""
        if root is None:
            check(self.L.stb_tindic_set_hroot(self.h, None))
            return
        root = np.ascontiguousarray(root, dtype=np.float64)
        if root.shape != (self.maxK,):
            raise StbError(f"expected {self.maxK} values, got shape {root.shape}")
        check(self.L.stb_tindic_set_hroot(self.h, dp(root)))

    def get_hroot(self):
        root = np.zeros(self.maxK, dtype=np.float64)
        check(self.L.stb_tindic_get_hroot(self.h, dp(root)))
        return root

    def sample_hgroups(self, alpha, gamma=1.0, seed: int = 0, sweep: int = 0, flags: int = 0, shape=1.0, scale=1.0):
        """one step of the grouped base weights: auxiliary tables, the root from Dirichlet(gamma + their sums), with
        HG_SAMPLE_ALPHA the concentration, then every group's h; alpha = 0 takes the concentration the last step left.
        Returns HGroupsInfo (alpha, tables, aux_tables).  Give it another seed than sample_lik"""
        keep, opts = hgroups_opts(alpha, gamma, shape, scale, flags, self.maxK)
        info = HGroupsInfo()
        rc = self.L.stb_tindic_sample_hgroups(self.h, C.byref(opts), seed, sweep, C.byref(info))
        if rc:
            err = StbError(last_error())
            err.info = info
            raise err
        return info

    # ---- base weights on a tree of nested groups (stb_tindic_set_htree / _set_htree_level / _get_htree_level / _sample_htree)

    def set_htree(self, off=None):
        """the tree: off[l] the contiguous ranges that cut level l (the restaurants for l = 0) into the nodes of level
        l + 1; None or an empty list removes it.  The rows of the levels >= 2 are set to the object's root"""
        offs = [np.ascontiguousarray(o, dtype=np.uint64) for o in (off or [])]
        L = len(offs)
        if not L:
            check(self.L.stb_tindic_set_htree(self.h, 0, None, None))
            self._htree_G = []
            return
        G = [int(o.shape[0]) - 1 for o in offs]
        check(self.L.stb_tindic_set_htree(self.h, L, (C.c_int * L)(*G), _ptr_array([o.ctypes.data for o in offs])))
        self._htree_G = G

    def set_htree_level(self, level: int, rows):
        """the rows of a level >= 2 (1-based): (G_level, maxK) positive values"""
        G = getattr(self, "_htree_G", [])
        if not 1 <= level <= len(G):
            raise StbError(f"level {level}: the tree has {len(G)} levels")
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        if rows.shape != (G[level - 1], self.maxK):
            raise StbError(f"expected shape {(G[level - 1], self.maxK)}, got {rows.shape}")
        check(self.L.stb_tindic_set_htree_level(self.h, level, dp(rows)))

    def get_htree_level(self, level: int):
        """a level's rows (G_level, maxK), after the queued work; level 1: what the last step drew"""
        G = getattr(self, "_htree_G", [])
        if not 1 <= level <= len(G):
            raise StbError(f"level {level}: the tree has {len(G)} levels")
        rows = np.zeros((G[level - 1], self.maxK), dtype=np.float64)
        check(self.L.stb_tindic_get_htree_level(self.h, level, dp(rows)))
        return rows

    def sample_htree(self, alpha, gamma=1.0, seed: int = 0, sweep: int = 0, flags: int = 0, shape=1.0, scale=1.0, levels=None):
        """one step of the base weights on the tree: auxiliary tables upwards, the root, with HT_SAMPLE_ALPHA every level's
        concentration, then the rows downwards; alpha one value a level (level 1 first), None: what the last step left.
        Returns HTreeInfo (alpha, tables, aux_tables a level).  Give it another seed than sample_lik"""
        L = len(getattr(self, "_htree_G", [])) if levels is None else levels
        keep, opts = htree_opts(L, alpha, gamma, shape, scale, flags, self.maxK)
        info = HTreeInfo()
        rc = self.L.stb_tindic_sample_htree(self.h, C.byref(opts), seed, sweep, C.byref(info))
        if rc:
            err = StbError(last_error())
            err.info = info
            raise err
        return info

    def loglik(self):
        """(sum over customers of log lik[class, dish], cells with customers and no likelihood) of the current state"""
        tot, imp = C.c_double(0.0), C.c_uint64(0)
        check(self.L.stb_tindic_loglik(self.h, C.byref(tot), C.byref(imp)))
        return tot.value, imp.value

    def get_h(self):
        """h[G] float64 (1 everywhere when none is set), after the queued work"""
        h = np.zeros(self.G, dtype=np.float64)
        check(self.L.stb_tindic_get_h(self.h, dp(h)))
        return h

    # ---- what the state predicts (stb_tindic_predict / _set_heldout / _heldout)

    def set_heldout(self, hoff=None, hcls=None):
        """the held-out customers of every restaurant: hoff[I+1] prefix sums and their classes hcls[hoff[I]]; None removes
        them.  Zeroes the accumulator and the sample count"""
        if hoff is None:
            check(self.L.stb_tindic_set_heldout(self.h, None, None))
            self.Hc = 0
            return
        hoff = np.ascontiguousarray(hoff, dtype=np.uint64)
        hcls = np.ascontiguousarray([] if hcls is None else hcls, dtype=np.uint32)
        if hoff.shape != (self.I + 1,) or hcls.shape[0] != int(hoff[-1]):
            raise StbError(f"TableIndicators.set_heldout: {hoff.shape[0]} offsets for {self.I} restaurants, "
                           f"{hcls.shape[0]} classes for {int(hoff[-1])} customers")
        check(self.L.stb_tindic_set_heldout(self.h, hoff.ctypes.data_as(C.POINTER(C.c_uint64)), hcls.ctypes.data_as(c_u32_p)))
        self.Hc = int(hoff[-1])

    def predict(self, a, bpar, tstride: int = 0):
        """theta (I, tstride) float64: every restaurant's predictive dish proportions in the current state (columns past
        K_i are 0); tstride 0: the largest K"""
        bpar = _bpar(bpar, self.I)
        tstride = int(tstride) or max(self.maxK, 1)
        theta = np.zeros((self.I, tstride), dtype=np.float64)
        check(self.L.stb_tindic_predict(self.h, float(a), dp(bpar), dp(theta), tstride))
        return theta

    def heldout(self, a, bpar, accumulate: bool = False, want_Hi: bool = True, flags=None):
        """(total, H_i[I] or None, PredictInfo): the held-out customers' log likelihood -- the current state's sum_c log p_c,
        or with accumulate the running estimate sum_c log(acc_c / S) after this state's p_c went into the accumulator"""
        bpar = _bpar(bpar, self.I)
        Hi = np.zeros(self.I, dtype=np.float64) if want_Hi else None
        tot, info = C.c_double(0.0), PredictInfo()
        fl = (PR_ACCUMULATE if accumulate else 0) if flags is None else int(flags)
        check(self.L.stb_tindic_heldout(self.h, float(a), dp(bpar), fl, C.byref(tot), None if Hi is None else dp(Hi),
                                        C.byref(info)))
        return tot.value, Hi, info

    # ---- the seating run forwards (stb_tindic_seat / _heldout_seq)

    def seat(self, a, bpar, seed: int, sweep: int):
        """(total, SeatInfo): the object's seating is forgotten and all its customers are seated in CSR order from empty
        restaurants, under its classes and matrix (the prior without); total = the sum of the restaurants' log weights"""
        bpar = _bpar(bpar, self.I)
        tot, info = C.c_double(0.0), SeatInfo()
        check(self.L.stb_tindic_seat(self.h, float(a), dp(bpar), seed, sweep, C.byref(tot), C.byref(info)))
        return tot.value, info

    # ---- customers' classes drawn from the matrix (stb_tindic_sample_classes / _generate / _get_classes)

    def sample_classes(self, seed: int, sweep: int, mask=None, want_info: bool = True):
        """every customer's class (mask: those with a non-zero byte) drawn from its dish's column of the matrix, behind the
        queued sweeps; an object without classes gets them.  Returns ClassesInfo after a wait, or None without one"""
        mp = None
        if mask is not None:
            mask = np.ascontiguousarray(mask, dtype=np.uint8)
            if mask.shape[0] != self.C:
                raise StbError(f"TableIndicators.sample_classes: {mask.shape[0]} mask bytes, {self.C} customers")
            mp = mask.ctypes.data_as(C.c_void_p)
        info = ClassesInfo() if want_info else None
        check(self.L.stb_tindic_sample_classes(self.h, mp, seed, sweep, None if info is None else C.byref(info)))
        self.rows = self.lik_device()[1]
        return info

    def generate(self, a, bpar, seed: int, sweep: int):
        """(SeatInfo, ClassesInfo): a draw of (z, t, cls) from the model given the matrix, h, a and b -- the seating of
        seat() under the prior, whatever matrix the object holds, then every class from its dish's column"""
        bpar = _bpar(bpar, self.I)
        si, ci = SeatInfo(), ClassesInfo()
        check(self.L.stb_tindic_generate(self.h, float(a), dp(bpar), seed, sweep, C.byref(si), C.byref(ci)))
        self.rows = self.lik_device()[1]
        return si, ci

    def get_classes(self):
        """(cls[C] uint32, rows) after the queued work"""
        cls = np.zeros(self.C, dtype=np.uint32)
        rows = C.c_uint(0)
        check(self.L.stb_tindic_get_classes(self.h, cls.ctypes.data_as(c_u32_p) if self.C else None, C.byref(rows)))
        return cls, rows.value

    # ---- Gaussian observations (stb_tindic_set_obs and what follows it in include/stb_hip.h)

    def set_obs(self, x=None):
        """x (C, D) float64: the object goes into observation mode (identity classes, a C x K matrix of ones); None: the
        observations, the classes and the matrix go"""
        if x is None:
            check(self.L.stb_tindic_set_obs(self.h, None, 0))
            self.obs_D = self.rows = self.stride = 0
            return
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.ndim != 2 or x.shape[0] != self.C:
            raise StbError(f"set_obs: x has shape {x.shape}; the object has {self.C} customers")
        check(self.L.stb_tindic_set_obs(self.h, dp(x), int(x.shape[1])))
        self.obs_D = int(x.shape[1])
        self.rows, self.stride = self.C, self.maxK      # (the identity classes and the C x K matrix)

    def set_gauss(self, mu, tau):
        """the dishes' means and precisions (K, D), and the matrix rewritten from them"""
        mu, tau = np.ascontiguousarray(mu, dtype=np.float64), np.ascontiguousarray(tau, dtype=np.float64)
        shape = (self.maxK, getattr(self, "obs_D", 0))
        if shape[1] and (mu.shape != shape or tau.shape != shape):
            raise StbError(f"set_gauss: mu {mu.shape}, tau {tau.shape}; expected {shape}")
        check(self.L.stb_tindic_set_gauss(self.h, dp(mu), dp(tau)))

    def get_gauss(self):
        """(mu, tau), each (K, D), after the queued work"""
        D = getattr(self, "obs_D", 0)
        mu, tau = np.zeros((self.maxK, max(D, 1))), np.zeros((self.maxK, max(D, 1)))
        check(self.L.stb_tindic_get_gauss(self.h, dp(mu), dp(tau)))
        return mu, tau

    def sample_gauss(self, prior, seed: int, sweep: int):
        """statistics, the draw of (mu, tau) and the matrix in one call (stb_tindic_sample_gauss); prior a GaussPrior or the
        pair gauss_prior returns.  Returns GaussInfo"""
        p = prior[0] if isinstance(prior, tuple) else prior
        info = GaussInfo()
        check(self.L.stb_tindic_sample_gauss(self.h, C.byref(p), seed, sweep, C.byref(info)))
        return info

    def gauss_loglik(self):
        tot = C.c_double(0.0)
        check(self.L.stb_tindic_gauss_loglik(self.h, C.byref(tot)))
        return tot.value

    def gauss_logml(self, prior):
        p = prior[0] if isinstance(prior, tuple) else prior
        tot = C.c_double(0.0)
        check(self.L.stb_tindic_gauss_logml(self.h, C.byref(p), C.byref(tot)))
        return tot.value

    # ---- held-out points under Gaussian observations (stb_tindic_set_heldout_obs / _gauss_heldout)

    def set_heldout_obs(self, hoff=None, y=None):
        """the held-out points of every restaurant: hoff[I+1] prefix sums and y (hoff[I], D); None removes them.  An empty
        accumulator, no samples"""
        if hoff is None:
            check(self.L.stb_tindic_set_heldout_obs(self.h, None, None))
            self.gHc = 0
            return
        hoff = np.ascontiguousarray(hoff, dtype=np.uint64)
        D = getattr(self, "obs_D", 0)
        y = np.ascontiguousarray(np.zeros((0, max(D, 1))) if y is None else y, dtype=np.float64)
        if hoff.shape != (self.I + 1,) or y.ndim != 2 or (D and y.shape != (int(hoff[-1]), D)):
            raise StbError(f"TableIndicators.set_heldout_obs: {hoff.shape[0]} offsets for {self.I} restaurants, y of shape "
                           f"{y.shape} for {int(hoff[-1])} points of {D} dimensions")
        check(self.L.stb_tindic_set_heldout_obs(self.h, hoff.ctypes.data_as(C.POINTER(C.c_uint64)), dp(y)))
        self.gHc = int(hoff[-1])

    def gauss_heldout(self, a, bpar, accumulate: bool = False, want_Hi: bool = True, want_resp: bool = False, flags=None):
        """(total, H_i[I] or None, resp (Hc, K) or None, PredictInfo): the held-out points' log predictive density under the
        current state, or with accumulate the running estimate sum_j log((1/S) sum_s p_j) after this state went into the
        log-domain accumulator"""
        bpar = _bpar(bpar, self.I)
        Hi = np.zeros(self.I, dtype=np.float64) if want_Hi else None
        resp = np.zeros((getattr(self, "gHc", 0), self.maxK), dtype=np.float64) if want_resp else None
        tot, info = C.c_double(0.0), PredictInfo()
        fl = (GH_ACCUMULATE if accumulate else 0) if flags is None else int(flags)
        check(self.L.stb_tindic_gauss_heldout(self.h, float(a), dp(bpar), fl, C.byref(tot), None if Hi is None else dp(Hi),
                                              None if resp is None else dp(resp), C.byref(info)))
        return tot.value, Hi, resp, info

    def gauss_heldout_reset(self):
        """an empty accumulator and no samples"""
        check(self.L.stb_tindic_gauss_heldout_reset(self.h))

    def gauss_heldout_get(self):
        """(M[Hc], A[Hc], the states accumulated): A e^M is the sum of the states' densities"""
        S = C.c_uint(0)
        n = getattr(self, "gHc", 0)
        M, A = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.float64)
        check(self.L.stb_tindic_gauss_heldout_get(self.h, dp(M) if n else None, dp(A) if n else None, C.byref(S)))
        return M, A, S.value

    def heldout_seq(self, a, bpar, particles: int, seed: int, sweep: int, want_Hi: bool = True):
        """(total, H_i[I] or None, SeatInfo): the held-out customers seated one after another on a private copy of every
        restaurant's state, `particles` times; H_i = log of the mean particle weight.  Writes nothing of the object"""
        bpar = _bpar(bpar, self.I)
        Hi = np.zeros(self.I, dtype=np.float64) if want_Hi else None
        tot, info = C.c_double(0.0), SeatInfo()
        check(self.L.stb_tindic_heldout_seq(self.h, float(a), dp(bpar), int(particles), seed, sweep, C.byref(tot),
                                            None if Hi is None else dp(Hi), C.byref(info)))
        return tot.value, Hi, info

    def heldout_pf(self, a, bpar, particles: int, tau: float, seed: int, sweep: int, want_Hi: bool = True):
        """(total, H_i[I] or None, PFInfo): heldout_seq's twin with resampling between customers (stb_seat_filter): at most
        64 particles, resampled when the effective sample size falls below tau * particles.  Writes nothing of the object"""
        bpar = _bpar(bpar, self.I)
        Hi = np.zeros(self.I, dtype=np.float64) if want_Hi else None
        tot, info = C.c_double(0.0), PFInfo()
        check(self.L.stb_tindic_heldout_pf(self.h, float(a), dp(bpar), int(particles), float(tau), seed, sweep, C.byref(tot),
                                           None if Hi is None else dp(Hi), C.byref(info)))
        return tot.value, Hi, info

    def heldout_ais(self, a, bpar, particles: int, S: int, seed: int, sweep: int, betas=None, passes: int = 1,
                    want_Hi: bool = True):
        """(total, H_i[I] or None, AISInfo): the held-out customers of an object that holds none of its own, scored by
        annealed importance sampling (stb_seat_anneal): S temperatures (betas: None for the even ladder), `passes` dish
        sweeps at each but the last.  Writes nothing of the object"""
        bpar = _bpar(bpar, self.I)
        Hi = np.zeros(self.I, dtype=np.float64) if want_Hi else None
        bp = None
        if betas is not None:
            betas = np.ascontiguousarray(betas, dtype=np.float64)
            bp = dp(betas)
        tot, info = C.c_double(0.0), AISInfo()
        check(self.L.stb_tindic_heldout_ais(self.h, float(a), dp(bpar), int(particles), int(S), bp, int(passes), seed, sweep,
                                            C.byref(tot), None if Hi is None else dp(Hi), C.byref(info)))
        return tot.value, Hi, info

    def heldout_reset(self):
        """zeroes the accumulator and the sample count"""
        check(self.L.stb_tindic_heldout_reset(self.h))

    def heldout_get(self):
        """(the accumulator p[Hc] float64, the states accumulated)"""
        S = C.c_uint(0)
        p = np.zeros(getattr(self, "Hc", 0), dtype=np.float64)
        check(self.L.stb_tindic_heldout_get(self.h, dp(p) if p.size else None, C.byref(S)))
        return p, S.value

    def free(self):
        if self.h:
            self.L.stb_tindic_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def sweep(tabs: DeviceTables, dg: DeviceGroups, stream=None):
    """out[d] = sum_{pairs, n>1} S_S_d(n,t)  (K3)"""
    torch = _torch()
    L = lib()
    wsb = int(L.stb_sweep_workspace_bytes(dg.G, tabs.D))
    ws = torch.empty(wsb, dtype=torch.uint8, device=tabs.tables.device)
    out = torch.empty(tabs.D, dtype=torch.float64, device=tabs.tables.device)
    check(L.stb_sweep_S(tabs.tables.data_ptr(), tabs.stride, tabs.S1.data_ptr(), tabs.N, tabs.D,
                        tabs.N, tabs.M, dg.n.data_ptr(), dg.t.data_ptr(), dg.G, out.data_ptr(),
                        ws.data_ptr(), wsb, stream_ptr(stream)))
    return out


def restaurant_terms(x, dg: DeviceGroups, stream=None):
    torch = _torch()
    L = lib()
    x = np.ascontiguousarray(np.atleast_1d(np.asarray(x, dtype=np.float64)))
    D = x.shape[0]
    wsb = int(L.stb_terms_workspace_bytes(dg.I, D))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dg.T.device)
    out = torch.empty(D, dtype=torch.float64, device=dg.T.device)
    check(L.stb_restaurant_terms(dp(x), D, dg.T.data_ptr(), dg.bpar.data_ptr(), dg.I, out.data_ptr(),
                                 ws.data_ptr(), wsb, stream_ptr(stream)))
    return out


def bterms(x, Q, shape, apar, dg: DeviceGroups, stream=None):
    torch = _torch()
    L = lib()
    x = np.ascontiguousarray(np.atleast_1d(np.asarray(x, dtype=np.float64)))
    J = x.shape[0]
    wsb = int(L.stb_terms_workspace_bytes(dg.I, J))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dg.T.device)
    out = torch.empty(J, dtype=torch.float64, device=dg.T.device)
    check(L.stb_bterms(dp(x), J, Q, shape, apar, dg.T.data_ptr(), dg.I, out.data_ptr(), ws.data_ptr(),
                       wsb, stream_ptr(stream)))
    return out
