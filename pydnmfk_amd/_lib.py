"""ctypes binding of libdnmf_hip.so (C ABI declared in include/dnmf.h).

There is NO CPU fallback: if the library is missing the import of this module fails
loudly, and every compute entry point requires CUDA(HIP) device pointers.
"""
import ctypes
import os

# torch bundles its own libamdhip64; it MUST be loaded first so that libdnmf_hip.so binds to the same HIP
# runtime instance (two runtimes in one process = "no ROCm-capable device" + foreign device pointers).
import torch  # noqa: F401  isort:skip

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdnmf_hip.so")

c_float_p = ctypes.c_void_p
c_long, c_int, c_float, c_size_t, c_void_p = ctypes.c_long, ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p

# name -> argtypes (restype is int unless listed in _RESTYPES); mirrors include/dnmf.h one to one
SIGNATURES = {
    "dnmf_last_error": [],
    "dnmf_version": [],
    "dnmf_kp": [c_int],
    "dnmf_ws_bytes": [c_long, c_long, c_int],
    "dnmf_gram_hht": [c_void_p, c_int, c_long, c_long, c_void_p, c_void_p, c_size_t, c_void_p],
    "dnmf_gram_wtw": [c_void_p, c_long, c_int, c_long, c_void_p, c_void_p, c_size_t, c_void_p],
    "dnmf_aht": [c_void_p, c_long, c_long, c_long, c_void_p, c_int, c_long, c_void_p, c_long, c_void_p],
    "dnmf_aht_hblocks": [c_void_p, c_long, c_long, c_long, c_void_p, c_long, c_int, c_void_p, c_long, c_void_p],
    "dnmf_wta": [c_void_p, c_long, c_long, c_long, c_void_p, c_int, c_long, c_void_p, c_long, c_void_p, c_size_t,
                 c_void_p],
    "dnmf_wta_gram": [c_void_p, c_long, c_long, c_long, c_void_p, c_int, c_long, c_void_p, c_long, c_void_p, c_void_p,
                      c_size_t, c_void_p],
    "dnmf_mu_update_w": [c_void_p, c_long, c_int, c_long, c_void_p, c_long, c_void_p, c_float, c_void_p],
    "dnmf_mu_update_h": [c_void_p, c_int, c_long, c_long, c_void_p, c_long, c_void_p, c_float, c_int, c_void_p],
    "dnmf_aht_update_w": [c_void_p, c_long, c_long, c_long, c_void_p, c_int, c_long, c_void_p, c_void_p, c_long,
                          c_float, c_void_p],
    "dnmf_mu_fro_step": [c_void_p, c_long, c_long, c_long, c_void_p, c_long, c_void_p, c_long, c_int, c_float, c_int,
                         c_int, c_void_p, c_size_t, c_void_p],
    "dnmf_mu_fro_onepass": [c_long, c_long, c_int],
    "dnmf_set_onepass": [c_int],
    "dnmf_set_persistent": [c_int],
    "dnmf_hals_w_col": [c_void_p, c_long, c_int, c_long, c_void_p, c_long, c_void_p, c_int, c_void_p, c_float, c_void_p,
                        c_void_p],
    "dnmf_hals_w_scale": [c_void_p, c_long, c_long, c_int, c_void_p, c_void_p],
    "dnmf_hals_update_w": [c_void_p, c_long, c_int, c_long, c_void_p, c_long, c_void_p, c_float, c_void_p, c_void_p],
    "dnmf_hals_sweep_w": [c_void_p, c_long, c_int, c_long, c_void_p, c_long, c_void_p, c_float, c_void_p, c_size_t, c_void_p],
    "dnmf_hals_sweep_status": [ctypes.POINTER(c_int), c_void_p],
    "dnmf_hals_sweep_plan": [c_long, c_int, c_long, c_long, c_int, c_int, c_void_p],      # out: int[6]
    "dnmf_hals_update_h": [c_void_p, c_int, c_long, c_long, c_void_p, c_long, c_void_p, c_float, c_void_p],
    "dnmf_kl_uht": [c_void_p, c_long, c_long, c_long, c_void_p, c_long, c_void_p, c_long, c_int, c_float, c_void_p,
                    c_long, c_void_p, c_size_t, c_void_p],
    "dnmf_kl_wtu": [c_void_p, c_long, c_long, c_long, c_void_p, c_long, c_void_p, c_long, c_int, c_float, c_void_p,
                    c_long, c_void_p, c_size_t, c_void_p],
    "dnmf_kl_uht_hblocks": [c_void_p, c_long, c_long, c_long, c_void_p, c_long, c_void_p, c_long, c_int, c_float, c_void_p,
                            c_long, c_void_p, c_size_t, c_void_p],
    "dnmf_rowsum": [c_void_p, c_int, c_long, c_long, c_void_p, c_void_p],
    "dnmf_colsum": [c_void_p, c_long, c_int, c_long, c_void_p, c_void_p, c_size_t, c_void_p],
    "dnmf_kl_update_w": [c_void_p, c_long, c_int, c_long, c_void_p, c_long, c_void_p, c_float, c_void_p],
    "dnmf_kl_update_h": [c_void_p, c_int, c_long, c_long, c_void_p, c_long, c_void_p, c_float, c_int, c_void_p],
    "dnmf_mu_kl_step": [c_void_p, c_long, c_long, c_long, c_void_p, c_long, c_void_p, c_long, c_int, c_float, c_int,
                        c_int, c_void_p, c_size_t, c_void_p],
    "dnmf_clamp_min": [c_void_p, c_long, c_long, c_long, c_float, c_void_p],
    "dnmf_scale_cols_div": [c_void_p, c_long, c_int, c_long, c_void_p, c_float, c_void_p],
    "dnmf_scale_rows_mul": [c_void_p, c_int, c_long, c_long, c_void_p, c_void_p],
    "dnmf_sqnorm": [c_void_p, c_long, c_long, c_long, c_void_p, c_void_p],
    "dnmf_clock_probe": [c_void_p, c_int, c_int, c_void_p],
    "dnmf_perturb_uniform": [c_void_p, c_void_p, c_long, c_long, c_long, c_long, c_float, ctypes.c_ulonglong, c_int, c_void_p],
    "dnmf_column_err": [c_void_p, c_long, c_long, c_long, c_void_p, c_long, c_void_p, c_long, c_int, c_void_p, c_void_p,
                        c_void_p],
    "dnmf_resid_sqnorm": [c_void_p, c_long, c_long, c_long, c_void_p, c_long, c_void_p, c_long, c_int, c_void_p,
                          c_void_p],
}
SIGNATURES["dnmf_resid_sqnorm_ws"] = SIGNATURES["dnmf_resid_sqnorm"][:-1] + [c_void_p, c_size_t, c_void_p]
# bf16 storage of A: same argument lists as the fp32 twins (A is passed as a device pointer either way)
for _n in ("aht", "wta", "wta_gram", "aht_update_w", "mu_fro_step", "sqnorm", "resid_sqnorm", "resid_sqnorm_ws", "column_err"):
    SIGNATURES["dnmf_%s_bf16a" % _n] = SIGNATURES["dnmf_" + _n]
# bf16x6 contractions: the fp32 argument lists, aht / aht_update_w with a workspace added
SIGNATURES["dnmf_ws_bytes_bf16x6"] = SIGNATURES["dnmf_ws_bytes"]
SIGNATURES["dnmf_aht_bf16x6"] = SIGNATURES["dnmf_aht"][:-1] + [c_void_p, c_size_t, c_void_p]
SIGNATURES["dnmf_wta_bf16x6"] = SIGNATURES["dnmf_wta"]
SIGNATURES["dnmf_aht_update_w_bf16x6"] = SIGNATURES["dnmf_aht_update_w"][:-1] + [c_void_p, c_size_t, c_void_p]
SIGNATURES["dnmf_mu_fro_step_bf16x6"] = SIGNATURES["dnmf_mu_fro_step"]
for _n in ("aht", "wta", "aht_update_w", "mu_fro_step"):
    SIGNATURES["dnmf_%s_bf16a_bf16x6" % _n] = SIGNATURES["dnmf_%s_bf16x6" % _n]
SIGNATURES["dnmf_kl_uht_bf16x6"] = SIGNATURES["dnmf_kl_uht"]
SIGNATURES["dnmf_kl_wtu_bf16x6"] = SIGNATURES["dnmf_kl_wtu"]
SIGNATURES["dnmf_mu_kl_step_bf16x6"] = SIGNATURES["dnmf_mu_kl_step"]
SIGNATURES["dnmf_bf16x6_plan"] = [c_long, c_long, c_int, c_long, c_int, c_int, c_void_p]      # m n k lda a_bf16 a_aligned16 out: long[12]
# grid exchanges inside the library (csrc/dnmf_comm.hip; the whole steps: csrc/dnmf_grid.hip); the communicator handle is an opaque pointer
SIGNATURES["dnmf_comm_unique_id"] = [c_void_p]
SIGNATURES["dnmf_comm_create"] = [c_void_p, c_int, c_int, c_int, c_int, ctypes.POINTER(c_void_p)]
COLLECTIVE_FN = ctypes.CFUNCTYPE(c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p)   # dnmf_collective_fn
SIGNATURES["dnmf_comm_create_hosted"] = [c_int, c_int, c_int, c_int, COLLECTIVE_FN, c_void_p, ctypes.POINTER(c_void_p)]
SIGNATURES["dnmf_comm_create_emulated"] = [c_int, c_int, c_int, ctypes.POINTER(c_void_p)]
SIGNATURES["dnmf_comm_destroy"] = [c_void_p]
SIGNATURES["dnmf_comm_rccl_version"] = [ctypes.POINTER(c_int), c_void_p, c_size_t]
SIGNATURES["dnmf_comm_direct_init"] = [c_void_p, c_size_t, c_void_p]
SIGNATURES["dnmf_comm_direct_connect"] = [c_void_p, c_void_p]
SIGNATURES["dnmf_comm_set_direct"] = [c_void_p, c_int]
SIGNATURES["dnmf_comm_direct_teardown"] = [c_void_p]
SIGNATURES["dnmf_comm_hals_xsweeps"] = [c_void_p, ctypes.POINTER(ctypes.c_ulonglong)]
SIGNATURES["dnmf_comm_set_direct_timeout"] = [c_void_p, ctypes.c_double]
SIGNATURES["dnmf_comm_fit_begin"] = [c_void_p]
DIRECT_HANDLE_BYTES = 80           # DNMF_DIRECT_HANDLE_BYTES
SIGNATURES["dnmf_comm_allreduce_direct"] = [c_void_p, c_void_p, c_size_t, c_void_p]
SIGNATURES["dnmf_comm_allreduce_direct_f64"] = [c_void_p, c_void_p, c_size_t, c_void_p]
SIGNATURES["dnmf_comm_direct_status"] = [c_void_p, ctypes.POINTER(c_int)]
SIGNATURES["dnmf_comm_info"] = [c_void_p, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int)]
SIGNATURES["dnmf_comm_set_overlap_chunks"] = [c_void_p, c_int]
SIGNATURES["dnmf_comm_set_always_exchange"] = [c_void_p, c_int]
SIGNATURES["dnmf_comm_set_null_exchange"] = [c_void_p, c_int]
SIGNATURES["dnmf_comm_allreduce"] = [c_void_p, c_void_p, c_size_t, c_int, c_void_p]
SIGNATURES["dnmf_ws_bytes_1d"] = SIGNATURES["dnmf_ws_bytes"]
SIGNATURES["dnmf_ws_bytes_2d"] = [c_long, c_long, c_int, c_int, c_int]
SIGNATURES["dnmf_hals_fro_step_1d"] = [c_void_p, c_long, c_long, c_long, c_void_p, c_long, c_void_p, c_long, c_int, c_float, c_int, c_int,
                                       c_int, c_void_p, c_size_t, c_void_p, c_void_p]
for _n in ("fro", "kl"):      # A, m_l, n_l, lda, W, m_w, ldw, H, n_h, ldh, k, eps, w_update, clamp, ws, ws_bytes, comm, stream
    SIGNATURES["dnmf_mu_%s_step_2d" % _n] = [c_void_p, c_long, c_long, c_long, c_void_p, c_long, c_long, c_void_p, c_long, c_long,
                                             c_int, c_float, c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p]
SIGNATURES["dnmf_hals_fro_step_2d"] = SIGNATURES["dnmf_mu_fro_step_2d"]
SIGNATURES["dnmf_mu_fro_step_1d"] = SIGNATURES["dnmf_mu_fro_step"][:-1] + [c_void_p, c_void_p]
SIGNATURES["dnmf_mu_kl_step_1d"] = SIGNATURES["dnmf_mu_fro_step_1d"]
SIGNATURES["dnmf_ws_bytes_hblocks"] = [c_long, c_long, c_int, c_long]
for _n in ("mu_fro_step_1d", "mu_fro_step_2d", "hals_fro_step_1d", "hals_fro_step_2d"):     # bf16-stored A: same argument lists
    SIGNATURES["dnmf_%s_bf16a" % _n] = SIGNATURES["dnmf_" + _n]
# whole fits (csrc/dnmf_fit.hip): A, m, n, lda, W, ldw, H, ldh, k, eps, w_update, itr, [column_sweep,] batch, a_stride, w_stride, h_stride,
# sq_out, ws, ws_bytes, stream
SIGNATURES["dnmf_ws_bytes_fit"] = [c_long, c_long, c_int, c_int]
SIGNATURES["dnmf_mu_fit_persistent"] = [c_long, c_long, c_int]
SIGNATURES["dnmf_hals_fit_persistent"] = [c_long, c_long, c_int]
SIGNATURES["dnmf_small_fit_plan"] = [c_int, c_int, c_int, c_long, c_long, c_int, c_void_p]      # method bf16 w_update m n k out: int[8]
SIGNATURES["dnmf_small_fit_launches"] = [c_void_p]                                              # out: unsigned long long[4]
SIGNATURES["dnmf_fit_set_timeout"] = [ctypes.c_double]
SIGNATURES["dnmf_mu_fro_fit"] = [c_void_p, c_long, c_long, c_long, c_void_p, c_long, c_void_p, c_long, c_int, c_float, c_int, c_int,
                                 c_int, c_long, c_long, c_long, c_void_p, c_void_p, c_size_t, c_void_p]
SIGNATURES["dnmf_mu_kl_fit"] = SIGNATURES["dnmf_mu_fro_fit"]
SIGNATURES["dnmf_mu_fro_fit_bf16a"] = SIGNATURES["dnmf_mu_fro_fit"]
SIGNATURES["dnmf_hals_fro_fit"] = SIGNATURES["dnmf_mu_fro_fit"][:12] + [c_int] + SIGNATURES["dnmf_mu_fro_fit"][12:]
SIGNATURES["dnmf_hals_fro_fit_bf16a"] = SIGNATURES["dnmf_hals_fro_fit"]
# the float64 path (csrc/dnmf_f64.hip)
c_double = ctypes.c_double
SIGNATURES["dnmf_f64_ws_bytes"] = [c_long, c_long, c_int]
SIGNATURES["dnmf_f64_aht"] = [c_void_p, c_long, c_long, c_long, c_void_p, c_int, c_long, c_void_p, c_long, c_void_p, c_size_t, c_void_p]
SIGNATURES["dnmf_f64_wta"] = SIGNATURES["dnmf_f64_aht"]
SIGNATURES["dnmf_f64_ws_bytes_fit"] = [c_long, c_long, c_int]
SIGNATURES["dnmf_f64_fit_tiny"] = [c_long, c_long, c_int, c_int]
SIGNATURES["dnmf_f64_fit"] = [c_int, c_void_p, c_long, c_long, c_long, c_void_p, c_long, c_void_p, c_long, c_int, c_double, c_int, c_int, c_void_p, c_void_p,
                              c_size_t, c_void_p]
SIGNATURES["dnmf_f64_mu_update_w"] = [c_void_p, c_long, c_int, c_long, c_void_p, c_long, c_void_p, c_long, c_double, c_void_p]
SIGNATURES["dnmf_f64_mu_update_h"] = [c_void_p, c_int, c_long, c_long, c_void_p, c_long, c_void_p, c_long, c_double, c_int, c_void_p]
SIGNATURES["dnmf_f64_kl_quot"] = [c_void_p, c_long, c_long, c_long, c_void_p, c_long, c_void_p, c_long, c_int, c_double, c_void_p, c_long, c_void_p]
for _n in ("dnmf_f64_kl_uht", "dnmf_f64_kl_wtu"):      # A m n lda W ldw H ldh k eps S lds U ws ws_bytes stream
    SIGNATURES[_n] = [c_void_p, c_long, c_long, c_long, c_void_p, c_long, c_void_p, c_long, c_int, c_double, c_void_p, c_long, c_void_p, c_void_p, c_size_t, c_void_p]
SIGNATURES["dnmf_f64_sqdiff"] = [c_void_p, c_long, c_long, c_long, c_void_p, c_long, c_void_p, c_long, c_int, c_void_p, c_long, c_void_p]
SIGNATURES["dnmf_f64_sum"] = [c_void_p, c_long, c_long, c_long, c_int, c_void_p, c_void_p, c_size_t, c_void_p]
SIGNATURES["dnmf_f64_colsum"] = SIGNATURES["dnmf_f64_sum"]
SIGNATURES["dnmf_f64_rowsum"] = [c_void_p, c_int, c_long, c_long, c_void_p, c_void_p]
SIGNATURES["dnmf_f64_ew"] = [c_int, c_void_p, c_long, c_long, c_long, c_void_p, c_long, c_void_p, c_double, c_int, c_void_p]
SIGNATURES["dnmf_f64_hals_w_col"] = [c_void_p, c_long, c_int, c_long, c_void_p, c_long, c_void_p, c_long, c_int, c_void_p, c_double, c_void_p,
                                     c_void_p, c_size_t, c_void_p]
SIGNATURES["dnmf_f64_hals_w_scale"] = [c_void_p, c_long, c_long, c_int, c_void_p, c_void_p]
SIGNATURES["dnmf_f64_hals_update_h"] = [c_void_p, c_int, c_long, c_long, c_void_p, c_long, c_void_p, c_long, c_double, c_void_p]
# host only: op m n k ld (long[4] or NULL) method out: long[12] (include/dnmf.h DNMF_F64_OP_*, DNMF_F64_FAM_*, DNMF_F64_PLAN_*)
SIGNATURES["dnmf_f64_plan"] = [c_int, c_long, c_long, c_int, c_void_p, c_int, c_void_p]
F64_OPS = ("aht", "wta", "kl_uht", "kl_wtu", "kl_quot", "sqdiff", "mu_update_w", "mu_update_h", "sum", "colsum", "ew", "fit")
F64_FAMILIES = ("none", "nt", "tn", "kl_uht", "kl_wtu", "nn_cols", "nn_rows", "upd_h", "sum", "colsum", "ew", "fit_tiny", "fit_chain", "image")
F64_PLAN_FIELDS = ("family", "nt", "rt", "vec", "full", "d", "count", "per", "v", "grid_x", "grid_y", "waves")
# host only: op bf16a m n k ld (long[4] or NULL) align (int[4] or NULL) ws_bytes ew_op out: long[26] (include/dnmf.h DNMF_DENSE_*)
SIGNATURES["dnmf_dense_plan"] = [c_int, c_int, c_long, c_long, c_int, c_void_p, c_void_p, c_size_t, c_int, c_void_p]
SIGNATURES["dnmf_dense_plan_variants"] = [c_void_p, c_int]      # rows: long[cap][10] or NULL; returns the number of rows
DENSE_VARIANT_FIELDS = ("family", "kt", "fast", "mode", "pf", "nt", "v", "edge", "ntemp", "bf16a")
DENSE_OPS = ("aht", "aht_hblocks", "aht_update_w", "wta", "wta_gram", "gram_hht", "gram_wtw", "mu_update_w", "mu_update_h", "ew",
             "kl_uht", "kl_uht_hblocks", "kl_wtu", "resid_sqnorm", "column_err", "sqnorm")
DENSE_FAMILIES = ("none", "nt16", "nt", "tn16", "tn16_gram", "tn", "update_w16", "update_w_seq", "update_h_seq", "ew", "wide",
                  "kl_uht_pipe", "kl_uht", "kl_wtu", "resid_lds", "resid", "colerr", "sqnorm", "kl16_uht", "kl16_wtu")
DENSE_PLAN_FIELDS = ("family", "kt", "fast", "mode", "pf", "nt", "v", "edge", "occ", "ntemp", "wfast", "grid_x", "grid_y", "block", "count", "per",
                     "reduce", "slices", "nk", "interior", "eligible", "b0_full", "b0_tail", "bl_full", "bl_tail", "aux")
DENSE_REDUCE = ("none", "single", "wide", "two_stage")
DENSE_EW_OPS = ("clamp_min", "scale_cols_div", "scale_rows_mul", "kl_update_h", "kl_update_w")
# BCD (csrc/dnmf_bcd.hip)
SIGNATURES["dnmf_bcd_state_init"] = [c_void_p, c_void_p, c_void_p]
SIGNATURES["dnmf_bcd_init_factor"] = [c_void_p, c_long, c_long, c_long, c_void_p, c_long, c_void_p, c_long, c_void_p, c_int, c_void_p]
SIGNATURES["dnmf_bcd_lipschitz"] = [c_void_p, c_int, c_void_p, c_int, c_void_p]
SIGNATURES["dnmf_bcd_ws_bytes_w"] = [c_long, c_int]
SIGNATURES["dnmf_bcd_update_w"] = [c_void_p, c_long, c_void_p, c_long, c_void_p, c_long, c_int, c_void_p, c_void_p, c_long, c_void_p,
                                   c_void_p, c_size_t, c_void_p]
SIGNATURES["dnmf_bcd_scale_cols"] = [c_void_p, c_long, c_int, c_long, c_void_p, c_void_p]
SIGNATURES["dnmf_bcd_update_h"] = [c_void_p, c_long, c_void_p, c_long, c_void_p, c_int, c_long, c_void_p, c_void_p, c_long, c_void_p]
SIGNATURES["dnmf_bcd_decide"] = [c_void_p, c_void_p, c_void_p]
SIGNATURES["dnmf_bcd_extrapolate"] = [c_void_p, c_long, c_void_p, c_long, c_void_p, c_long, c_long, c_void_p, c_long, c_void_p, c_long,
                                      c_void_p, c_long, c_long, c_int, c_void_p, c_long, c_void_p, c_long, c_void_p, c_void_p, c_void_p,
                                      c_void_p]
SIGNATURES["dnmf_bcd_ws_bytes"] = [c_long, c_long, c_int]
SIGNATURES["dnmf_bcd_ws_bytes_fit"] = [c_long, c_long, c_int, c_int]
SIGNATURES["dnmf_bcd_fro_fit"] = SIGNATURES["dnmf_mu_fro_fit"]
# sparse data block (csrc/dnmf_csr.hip): rowptr col val rows ... long_rows long_segptr n_long nseg ws ws_bytes stream
SIGNATURES["dnmf_csr_kpad"] = [c_int]
SIGNATURES["dnmf_csr_seg"] = []
SIGNATURES["dnmf_csr_ws_bytes"] = [c_long, c_long, c_int, c_int]
SIGNATURES["dnmf_csr_pack"] = [c_void_p, c_long, c_long, c_long, c_int, c_void_p, c_void_p]
SIGNATURES["dnmf_csr_mm"] = [c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_int, c_void_p, c_long, c_int, c_void_p, c_void_p, c_int, c_int,
                             c_void_p, c_size_t, c_void_p]
SIGNATURES["dnmf_csr_kl_mm"] = [c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_int, c_float, c_void_p, c_long, c_int, c_void_p,
                                c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p]
SIGNATURES["dnmf_csr_resid_sqnorm"] = [c_void_p, c_void_p, c_void_p, c_long, c_long, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int,
                                       c_void_p, c_void_p, c_size_t, c_void_p]
# ... whose unstored entries are missing: rowptr col val rows Lp Fp k eps kl [clamp] out(s) ld out_trans + the long-row tail
SIGNATURES["dnmf_csr_masked_ws_bytes"] = [c_long, c_long, c_int, c_int]
SIGNATURES["dnmf_csr_masked_mm"] = [c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_int, c_float, c_int, c_void_p, c_void_p, c_long,
                                    c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p]
SIGNATURES["dnmf_csr_masked_update"] = [c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_int, c_float, c_int, c_int, c_void_p, c_long,
                                        c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p]
SIGNATURES["dnmf_csr_ratio_update"] = [c_void_p, c_long, c_long, c_long, c_void_p, c_void_p, c_long, c_float, c_int, c_void_p]
SIGNATURES["dnmf_csr_masked_resid_sqnorm"] = SIGNATURES["dnmf_csr_resid_sqnorm"]
# NMFk on a sparse block: rowptr col val rows ncols transposed noise_var seed val_out stream
SIGNATURES["dnmf_csr_perturb_uniform"] = [c_void_p, c_void_p, c_void_p, c_long, c_long, c_int, c_float, ctypes.c_ulonglong, c_void_p, c_void_p]
SIGNATURES["dnmf_csr_column_err_ws_bytes"] = [c_long, c_long, c_int, c_int, c_int]
SIGNATURES["dnmf_csr_column_err"] = [c_void_p, c_void_p, c_void_p, c_long, c_long, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_int,
                                     c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
# dense data with NaN = not observed (csrc/dnmf_masked.hip): A m n lda W ldw H ldh k eps kl [clamp] [num den ldo] ws ws_bytes stream
SIGNATURES["dnmf_masked_ws_bytes"] = [c_long, c_long, c_int]
SIGNATURES["dnmf_masked_plan"] = [c_long, c_long, c_int, c_void_p]      # out: long[6]
SIGNATURES["dnmf_masked_reduce_grid"] = [c_long, c_long]
SIGNATURES["dnmf_masked_aht_pair"] = [c_void_p, c_long, c_long, c_long, c_void_p, c_long, c_void_p, c_long, c_int, c_float, c_int, c_void_p, c_void_p,
                                      c_long, c_void_p, c_size_t, c_void_p]
SIGNATURES["dnmf_masked_wta_pair"] = SIGNATURES["dnmf_masked_aht_pair"]
SIGNATURES["dnmf_masked_update_w"] = [c_void_p, c_long, c_long, c_long, c_void_p, c_long, c_void_p, c_long, c_int, c_float, c_int, c_void_p, c_size_t,
                                      c_void_p]
SIGNATURES["dnmf_masked_update_h"] = [c_void_p, c_long, c_long, c_long, c_void_p, c_long, c_void_p, c_long, c_int, c_float, c_int, c_int, c_void_p,
                                      c_size_t, c_void_p]
SIGNATURES["dnmf_masked_resid_sqnorm"] = [c_void_p, c_long, c_long, c_long, c_void_p, c_long, c_void_p, c_long, c_int, c_void_p, c_void_p]
SIGNATURES["dnmf_masked_sqnorm"] = [c_void_p, c_long, c_long, c_long, c_void_p, c_void_p]
# the masked per-column error (NMFk) and the whole masked fit: A m n lda W ldw H ldh k ...
SIGNATURES["dnmf_masked_column_err_ws_bytes"] = [c_long, c_long, c_int]
SIGNATURES["dnmf_masked_column_err_plan"] = [c_long, c_long, c_int, c_void_p]      # out: long[3]
SIGNATURES["dnmf_masked_column_err"] = [c_void_p, c_long, c_long, c_long, c_void_p, c_long, c_void_p, c_long, c_int, c_void_p, c_void_p, c_void_p,
                                        c_size_t, c_void_p]
SIGNATURES["dnmf_masked_ws_bytes_fit"] = [c_long, c_long, c_int]
SIGNATURES["dnmf_masked_mu_fit"] = [c_void_p, c_long, c_long, c_long, c_void_p, c_long, c_void_p, c_long, c_int, c_float, c_int, c_int, c_int,
                                    c_void_p, c_void_p, c_size_t, c_void_p]
# the Itakura-Saito rule (csrc/dnmf_is.hip): A m n lda W ldw H ldh k eps [clamp] [num den ldo] ws ws_bytes stream
SIGNATURES["dnmf_is_ws_bytes"] = [c_long, c_long, c_int]
SIGNATURES["dnmf_is_ws_bytes_fit"] = [c_long, c_long, c_int]
SIGNATURES["dnmf_is_plan"] = [c_long, c_long, c_int, c_void_p]      # out: long[8]
SIGNATURES["dnmf_is_aht_pair"] = [c_void_p, c_long, c_long, c_long, c_void_p, c_long, c_void_p, c_long, c_int, c_float, c_void_p, c_void_p, c_long,
                                  c_void_p, c_size_t, c_void_p]
SIGNATURES["dnmf_is_wta_pair"] = SIGNATURES["dnmf_is_aht_pair"]
SIGNATURES["dnmf_is_update_w"] = [c_void_p, c_long, c_long, c_long, c_void_p, c_long, c_void_p, c_long, c_int, c_float, c_void_p, c_size_t, c_void_p]
SIGNATURES["dnmf_is_update_h"] = [c_void_p, c_long, c_long, c_long, c_void_p, c_long, c_void_p, c_long, c_int, c_float, c_int, c_void_p, c_size_t,
                                  c_void_p]
SIGNATURES["dnmf_is_ratio_update"] = [c_void_p, c_long, c_long, c_long, c_void_p, c_void_p, c_long, c_float, c_int, c_void_p]
SIGNATURES["dnmf_is_divergence"] = [c_void_p, c_long, c_long, c_long, c_void_p, c_long, c_void_p, c_long, c_int, c_float, c_void_p, c_void_p, c_size_t,
                                    c_void_p]
SIGNATURES["dnmf_is_mu_fit"] = [c_void_p, c_long, c_long, c_long, c_void_p, c_long, c_void_p, c_long, c_int, c_float, c_int, c_int, c_void_p, c_void_p,
                                c_size_t, c_void_p]
# the per-column Itakura-Saito divergence (NMFk under norm='is'): A m n lda W ldw H ldh k eps div ws ws_bytes stream
SIGNATURES["dnmf_is_column_div_ws_bytes"] = [c_long, c_long, c_int]
SIGNATURES["dnmf_is_column_div_plan"] = [c_long, c_long, c_int, c_void_p]      # out: long[3]
SIGNATURES["dnmf_is_column_div"] = SIGNATURES["dnmf_is_divergence"]
# the beta-divergence rule (csrc/dnmf_beta.hip): the Itakura-Saito signatures with `float beta` after eps.  A table of its own: the
# core table above is held, entry point by entry point, to the workspace contract by tests/test_workspace_cpu.py, tests/test_capi.py and
# tests/test_gpu_workspace.py; this family's entries are held to the same contract by tests/test_beta_workspace_cpu.py and
# tests/test_gpu_beta_workspace.py
BETA_SIGNATURES = {}
BETA_SIGNATURES["dnmf_beta_ws_bytes"] = [c_long, c_long, c_int]
BETA_SIGNATURES["dnmf_beta_ws_bytes_fit"] = [c_long, c_long, c_int]
BETA_SIGNATURES["dnmf_beta_plan"] = [c_long, c_long, c_int, c_void_p]      # out: long[8]
for _name in ("aht_pair", "wta_pair", "update_w", "update_h", "divergence", "mu_fit"):
    _sig = SIGNATURES["dnmf_is_" + _name]
    BETA_SIGNATURES["dnmf_beta_" + _name] = _sig[:10] + [c_float] + _sig[10:]
BETA_SIGNATURES["dnmf_beta_ratio_update"] = SIGNATURES["dnmf_is_ratio_update"][:8] + [c_float] + SIGNATURES["dnmf_is_ratio_update"][8:]
# the per-column statistic of an NMFk sweep under norm='beta' (include/dnmf_beta_nmfk_api.h), a table of its own as well (the table above
# is pinned to the ten functions of include/dnmf_beta_api.h): A m n lda W ldw H ldh k eps beta div pw ws ws_bytes stream
BETA_NMFK_SIGNATURES = {}
BETA_NMFK_SIGNATURES["dnmf_beta_column_div_ws_bytes"] = [c_long, c_long, c_int]
BETA_NMFK_SIGNATURES["dnmf_beta_column_div_plan"] = [c_long, c_long, c_int, c_void_p]      # out: long[3]
BETA_NMFK_SIGNATURES["dnmf_beta_column_div"] = BETA_SIGNATURES["dnmf_beta_divergence"][:12] + [c_void_p] + BETA_SIGNATURES["dnmf_beta_divergence"][12:]
# the W phase from a transposed image of A (csrc/dnmf_timg.hip): build A m n lda At ldat stream; bind the same without the stream
SIGNATURES["dnmf_wimage_bytes"] = [c_long, c_long]
SIGNATURES["dnmf_wimage_build"] = [c_void_p, c_long, c_long, c_long, c_void_p, c_long, c_void_p]
SIGNATURES["dnmf_wimage_bind"] = [c_void_p, c_long, c_long, c_long, c_void_p, c_long]
SIGNATURES["dnmf_wimage_unbind"] = []
SIGNATURES["dnmf_set_wimage"] = [c_int]
SIGNATURES["dnmf_wimage_plan"] = [c_long, c_long, c_int, c_long, c_int, c_int, c_void_p]      # out: int[6]
_RESTYPES = {"dnmf_beta_column_div_ws_bytes": c_size_t, "dnmf_beta_ws_bytes": c_size_t, "dnmf_beta_ws_bytes_fit": c_size_t, "dnmf_is_column_div_ws_bytes": c_size_t, "dnmf_is_ws_bytes": c_size_t,"dnmf_is_ws_bytes_fit": c_size_t, "dnmf_wimage_bytes": c_size_t, "dnmf_wimage_unbind": None, "dnmf_masked_column_err_ws_bytes": c_size_t, "dnmf_masked_ws_bytes_fit": c_size_t, "dnmf_masked_ws_bytes": c_size_t,"dnmf_masked_reduce_grid": c_long, "dnmf_csr_column_err_ws_bytes": c_size_t, "dnmf_csr_masked_ws_bytes": c_size_t, "dnmf_csr_ws_bytes": c_size_t, "dnmf_ws_bytes_fit": c_size_t, "dnmf_f64_ws_bytes": c_size_t, "dnmf_f64_ws_bytes_fit": c_size_t, "dnmf_last_error": ctypes.c_char_p, "dnmf_ws_bytes": c_size_t, "dnmf_ws_bytes_bf16x6": c_size_t,
             "dnmf_ws_bytes_1d": c_size_t, "dnmf_ws_bytes_hblocks": c_size_t, "dnmf_ws_bytes_2d": c_size_t,
             "dnmf_bcd_ws_bytes_w": c_size_t, "dnmf_bcd_ws_bytes": c_size_t, "dnmf_bcd_ws_bytes_fit": c_size_t}


def load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "pydnmfk_amd: %s not found. Build it with `python -m pydnmfk_amd.build` (hipcc, gfx950). "
            "There is no CPU fallback." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, args in list(SIGNATURES.items()) + list(BETA_SIGNATURES.items()) + list(BETA_NMFK_SIGNATURES.items()):
        fn = getattr(lib, name)  # AttributeError if the ABI drifted from include/dnmf.h
        fn.argtypes = args
        fn.restype = _RESTYPES.get(name, c_int)
    return lib


lib = load()


class DnmfError(RuntimeError):
    pass


class PersistentTimeout(DnmfError):
    """A kernel whose workgroups wait for each other gave up (dnmf_hals_sweep_status): its workgroups were not all resident -- the GPU is
    shared with another process or stream.  The factors it was working on are invalid."""


def check(rc):
    if rc != 0:
        raise DnmfError("libdnmf_hip: %s (code %d)" % (lib.dnmf_last_error().decode(), rc))


def f64_plan(op, m, n, k, ld=(), method=0):
    """dnmf_f64_plan as a dict: which kernel the float64 entry point `op` (a name of F64_OPS) launches for the shape -- `family` by
    name, the other F64_PLAN_FIELDS as integers.  ld: the pitches in the order of the entry point's arguments (missing: packed)."""
    pitches = (c_long * 4)(*(list(ld) + [0] * (4 - len(ld))))
    out = (c_long * len(F64_PLAN_FIELDS))()
    check(lib.dnmf_f64_plan(F64_OPS.index(op), int(m), int(n), int(k), pitches, int(method), out))
    p = dict(zip(F64_PLAN_FIELDS, out))
    p["family"] = F64_FAMILIES[p["family"]]
    return p


def dense_plan(op, m, n, k, ld=(), align=(), bf16a=False, ws_bytes=None, ew_op="clamp_min"):
    """dnmf_dense_plan as a dict: which kernel the float32 entry point `op` (a name of DENSE_OPS) launches for the shape -- `family` and
    `reduce` by name, the other DENSE_PLAN_FIELDS as integers.  ld / align: the pitches (elements) and the addresses modulo 16 (bytes) of
    the operands in the order include/dnmf.h gives for the op (missing: packed / aligned).  ws_bytes: None = dnmf_ws_bytes(m, n, k)."""
    pitches = (c_long * 4)(*(list(ld) + [0] * (4 - len(ld))))
    offs = (c_int * 4)(*(list(align) + [0] * (4 - len(align))))
    out = (c_long * len(DENSE_PLAN_FIELDS))()
    if ws_bytes is None:
        ws_bytes = lib.dnmf_ws_bytes(int(m), int(n), int(k)) if op != "ew" else 0
    check(lib.dnmf_dense_plan(DENSE_OPS.index(op), int(bool(bf16a)), int(m), int(n), int(k), pitches, offs, int(ws_bytes),
                              DENSE_EW_OPS.index(ew_op), out))
    p = dict(zip(DENSE_PLAN_FIELDS, out))
    p["family"] = DENSE_FAMILIES[p["family"]]
    p["reduce"] = DENSE_REDUCE[p["reduce"]]
    return p


def dense_plan_variants():
    """dnmf_dense_plan_variants as a set of tuples in the order of DENSE_VARIANT_FIELDS (family by name)"""
    n = lib.dnmf_dense_plan_variants(None, 0)
    rows = (c_long * (n * len(DENSE_VARIANT_FIELDS)))()
    assert lib.dnmf_dense_plan_variants(rows, n) == n
    w = len(DENSE_VARIANT_FIELDS)
    return {(DENSE_FAMILIES[rows[i * w]],) + tuple(rows[i * w + 1:(i + 1) * w]) for i in range(n)}
