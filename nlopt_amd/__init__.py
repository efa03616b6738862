"""nlopt_amd — Python face of libnlopt_amd.so, the MI355X-native drop-in for NLopt's stochastic
population-based global optimisers (CRS2_LM / ISRES / MLSL).

The product is the C-ABI shared library (include/nlopt.h + include/nlopt_amd.h); this module only
loads it with ctypes: `Opt` is the thin face the tests and bench.py use (traces, statistics, communicators, device
buffers for the kernel-level tests); nlopt_amd/nlopt.py is the full mirror of the reference's Python module
(`import nlopt`: src/swig/nlopt.i, nlopt-python.i) for programs written against that.
There is no CPU implementation behind it: without a visible HIP device `optimize` raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NLOPT_AMD_LIB") or os.path.join(_HERE, "lib", "libnlopt_amd.so")    # NLOPT_AMD_LIB: an instrumented build (tools/)

# nlopt_algorithm values (include/nlopt.h; ABI)
GN_CRS2_LM, GN_MLSL, GD_MLSL, GN_MLSL_LDS, GD_MLSL_LDS = 19, 20, 21, 22, 23
LD_LBFGS, LD_MMA, GN_ISRES, G_MLSL, G_MLSL_LDS, GN_ESCH = 11, 24, 35, 38, 39, 42
LN_COBYLA, LN_NELDERMEAD, LN_SBPLX = 25, 28, 29
LD_TNEWTON, LD_TNEWTON_RESTART, LD_TNEWTON_PRECOND, LD_TNEWTON_PRECOND_RESTART = 15, 16, 17, 18
# nlopt_result values
FAILURE, INVALID_ARGS, OUT_OF_MEMORY, ROUNDOFF_LIMITED, FORCED_STOP = -1, -2, -3, -4, -5
SUCCESS, STOPVAL_REACHED, FTOL_REACHED, XTOL_REACHED, MAXEVAL_REACHED, MAXTIME_REACHED = 1, 2, 3, 4, 5, 6

OBJECTIVES = {"rastrigin": 0, "ackley": 1, "griewank": 2, "rosenbrock": 3, "levy": 4, "sphere": 5}

NLOPT_FUNC = C.CFUNCTYPE(C.c_double, C.c_uint, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p)
NLOPT_MFUNC = C.CFUNCTYPE(None, C.c_uint, C.POINTER(C.c_double), C.c_uint, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p)

TRACE_DTYPE = np.dtype([("f", "f8"), ("row", "i8"), ("kind", "i4"), ("accepted", "i4")])


class Stats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("rounds", "slots_launched", "slots_used", "slots_invalid", "slots_newbest",
                                           "slots_role", "evals_init", "evals_trial", "evals_mutation", "accepted",
                                           "mt_words")] + \
               [("t_init_s", C.c_double), ("t_trial_s", C.c_double), ("t_gather_ms", C.c_double),
                ("gather_launches", C.c_uint64), ("gather_bytes", C.c_uint64), ("generations", C.c_uint64),
                ("rank_sweeps", C.c_uint64), ("t_eval_s", C.c_double), ("t_rank_s", C.c_double), ("t_evolve_s", C.c_double),
                ("t_rng_s", C.c_double), ("lbfgs_launches", C.c_uint64), ("lbfgs_bytes", C.c_uint64), ("t_lbfgs_ms", C.c_double),
                ("t_stochrank_ms", C.c_double), ("stochrank_launches", C.c_uint64), ("stochrank_ticks", C.c_uint64),
                ("t_allgather_ms", C.c_double), ("allgather_bytes", C.c_uint64),
                ("evolve_rounds_enqueued", C.c_uint64), ("evolve_rounds", C.c_uint64),
                ("t_engine_s", C.c_double), ("t_walk_s", C.c_double),
                ("list_refreshes", C.c_uint64), ("list_refreshes_beside_device", C.c_uint64), ("t_list_refresh_s", C.c_double),
                ("isres_gate_timeouts", C.c_uint64), ("mlsl_sampled_ahead", C.c_uint64), ("cobyla_host_searches", C.c_uint64), ("lbfgs_longest_chain_steps", C.c_uint64), ("mlsl_gate_timeouts", C.c_uint64),
                ("isres_usercon_launches", C.c_uint64)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


_lib = None


def build(force=False, verbose=False):
    from . import _build as _b
    return _b.build(force=force, verbose=verbose)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def lib():
    """the loaded C-ABI library with argtypes set; raises if it has not been built"""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libnlopt_amd.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
    L = C.CDLL(LIB_PATH)
    vp, dbl, dpp = C.c_void_p, C.c_double, C.POINTER(C.c_double)
    L.nlopt_create.restype = vp
    L.nlopt_create.argtypes = [C.c_int, C.c_uint]
    L.nlopt_copy.restype = vp
    L.nlopt_copy.argtypes = [vp]
    L.nlopt_destroy.argtypes = [vp]
    L.nlopt_destroy.restype = None
    L.nlopt_optimize.argtypes = [vp, dpp, dpp]
    for nm in ("nlopt_set_min_objective", "nlopt_set_max_objective"):
        getattr(L, nm).argtypes = [vp, vp, vp]
    for nm in ("nlopt_set_lower_bounds", "nlopt_set_upper_bounds", "nlopt_get_lower_bounds", "nlopt_get_upper_bounds",
               "nlopt_set_xtol_abs", "nlopt_get_xtol_abs", "nlopt_set_x_weights", "nlopt_get_x_weights",
               "nlopt_set_initial_step"):
        getattr(L, nm).argtypes = [vp, dpp]
    for nm in ("nlopt_set_lower_bounds1", "nlopt_set_upper_bounds1", "nlopt_set_stopval", "nlopt_set_ftol_rel",
               "nlopt_set_ftol_abs", "nlopt_set_xtol_rel", "nlopt_set_xtol_abs1", "nlopt_set_x_weights1",
               "nlopt_set_maxtime", "nlopt_set_initial_step1"):
        getattr(L, nm).argtypes = [vp, dbl]
    for nm in ("nlopt_get_stopval", "nlopt_get_ftol_rel", "nlopt_get_ftol_abs", "nlopt_get_xtol_rel", "nlopt_get_maxtime"):
        getattr(L, nm).argtypes = [vp]
        getattr(L, nm).restype = dbl
    L.nlopt_set_lower_bound.argtypes = [vp, C.c_int, dbl]
    L.nlopt_set_upper_bound.argtypes = [vp, C.c_int, dbl]
    L.nlopt_set_maxeval.argtypes = [vp, C.c_int]
    for nm in ("nlopt_get_maxeval", "nlopt_get_numevals", "nlopt_get_force_stop", "nlopt_force_stop", "nlopt_get_algorithm"):
        getattr(L, nm).argtypes = [vp]
    L.nlopt_set_force_stop.argtypes = [vp, C.c_int]
    L.nlopt_get_dimension.argtypes = [vp]
    L.nlopt_get_dimension.restype = C.c_uint
    L.nlopt_set_population.argtypes = [vp, C.c_uint]
    L.nlopt_get_population.argtypes = [vp]
    L.nlopt_get_population.restype = C.c_uint
    L.nlopt_set_vector_storage.argtypes = [vp, C.c_uint]
    L.nlopt_get_vector_storage.argtypes = [vp]
    L.nlopt_get_vector_storage.restype = C.c_uint
    L.nlopt_set_local_optimizer.argtypes = [vp, vp]
    L.nlopt_get_errmsg.argtypes = [vp]
    L.nlopt_get_errmsg.restype = C.c_char_p
    L.nlopt_set_param.argtypes = [vp, C.c_char_p, dbl]
    L.nlopt_get_param.argtypes = [vp, C.c_char_p, dbl]
    L.nlopt_get_param.restype = dbl
    L.nlopt_has_param.argtypes = [vp, C.c_char_p]
    L.nlopt_num_params.argtypes = [vp]
    L.nlopt_num_params.restype = C.c_uint
    L.nlopt_nth_param.argtypes = [vp, C.c_uint]
    L.nlopt_nth_param.restype = C.c_char_p
    for nm in ("nlopt_add_inequality_constraint", "nlopt_add_equality_constraint"):
        getattr(L, nm).argtypes = [vp, vp, vp, dbl]
    for nm in ("nlopt_remove_inequality_constraints", "nlopt_remove_equality_constraints"):
        getattr(L, nm).argtypes = [vp]
    L.nlopt_srand.argtypes = [C.c_ulong]
    L.nlopt_srand.restype = None
    L.nlopt_algorithm_name.argtypes = [C.c_int]
    L.nlopt_algorithm_name.restype = C.c_char_p
    L.nlopt_algorithm_to_string.argtypes = [C.c_int]
    L.nlopt_algorithm_to_string.restype = C.c_char_p
    L.nlopt_algorithm_from_string.argtypes = [C.c_char_p]
    L.nlopt_result_to_string.argtypes = [C.c_int]
    L.nlopt_result_to_string.restype = C.c_char_p
    L.nlopt_result_from_string.argtypes = [C.c_char_p]
    L.nlopt_version.argtypes = [C.POINTER(C.c_int)] * 3
    L.nlopt_urand.argtypes = [dbl, dbl]
    L.nlopt_urand.restype = dbl
    L.nlopt_nrand.argtypes = [dbl, dbl]
    L.nlopt_nrand.restype = dbl
    L.nlopt_iurand.argtypes = [C.c_int]
    L.nla_genrand_int32.restype = C.c_uint32
    # extension
    L.nlopt_amd_objective.argtypes = [C.c_int]
    L.nlopt_amd_objective.restype = vp
    L.nlopt_amd_objective_id.argtypes = [vp]
    L.nlopt_amd_objective_name.argtypes = [C.c_int]
    L.nlopt_amd_objective_name.restype = C.c_char_p
    L.nlopt_amd_objective_box.argtypes = [C.c_int, dpp, dpp]
    L.nlopt_amd_objective_box.restype = None
    L.nlopt_amd_constraint_blocksum.restype = vp
    L.nlopt_amd_set_trace.argtypes = [vp, vp, C.c_size_t]
    L.nlopt_amd_trace_len.argtypes = [vp]
    L.nlopt_amd_trace_len.restype = C.c_size_t
    L.nlopt_amd_get_stats.argtypes = [vp, C.POINTER(Stats)]
    L.nlopt_amd_crs_open.argtypes = [vp, dpp, dpp, C.POINTER(C.c_int)]
    L.nlopt_amd_crs_open.restype = vp
    L.nlopt_amd_crs_step.argtypes = [vp, C.c_long]
    L.nlopt_amd_crs_close.argtypes = [vp]
    # device runtime + kernel-level C-ABI
    L.nla_dev_malloc.argtypes = [C.c_size_t]
    L.nla_dev_malloc.restype = vp
    L.nla_dev_free.argtypes = [vp]
    L.nla_dev_free.restype = None
    for nm in ("nla_memcpy_h2d", "nla_memcpy_d2h", "nla_memcpy_d2d"):
        getattr(L, nm).argtypes = [vp, vp, C.c_size_t, vp]
    L.nla_memset.argtypes = [vp, C.c_int, C.c_size_t, vp]
    L.nla_stream_create.restype = vp
    L.nla_stream_destroy.argtypes = [vp]
    L.nla_stream_sync.argtypes = [vp]
    L.nla_event_create.restype = vp
    L.nla_event_destroy.argtypes = [vp]
    L.nla_event_record.argtypes = [vp, vp]
    L.nla_event_sync.argtypes = [vp]
    L.nla_event_elapsed_ms.argtypes = [vp, vp]
    L.nla_event_elapsed_ms.restype = C.c_float
    L.nla_dev_error_string.argtypes = [C.c_int]
    L.nla_dev_error_string.restype = C.c_char_p
    L.nla_mtstream_create.argtypes = [vp]
    L.nla_mtstream_create.restype = vp
    L.nla_mtstream_destroy.argtypes = [vp]
    L.nla_mtstream_destroy.restype = None
    L.nla_mtstream_fill.argtypes = [vp, C.c_uint64, C.c_uint64, vp]
    L.nla_mtstream_finish.argtypes = [vp, C.c_uint64]
    L.nla_mtstream_rankbits.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int64, C.c_int64, vp]
    L.nla_k_mt_jump.argtypes = [vp, vp, vp, C.c_int, vp]
    L.nla_k_mt_generate.argtypes = [vp, C.c_uint64, C.c_int, C.c_uint64, C.c_uint64, vp, vp]
    L.nla_k_crs_init_rows.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int64, C.c_int64, vp, vp, vp]
    L.nla_k_eval.argtypes = [C.c_int, C.c_int, C.c_int, vp, C.c_int64, vp, vp]
    L.nla_k_crs_vitter.argtypes = [C.c_int, C.c_int64, vp, C.c_int, vp, vp, vp, vp]
    L.nla_k_crs_advance.argtypes = [C.c_int, C.c_int, vp, C.c_int64, vp, vp, vp, C.c_uint32, C.c_uint64, C.c_int, vp, C.c_int,
                                    vp, vp, C.c_int, vp, vp, vp, C.c_int, vp]
    L.nlopt_amd_has_device_objective.argtypes = [vp]
    for nm in ("nlopt_amd_add_inequality_device_mconstraint", "nlopt_amd_add_equality_device_mconstraint"):
        getattr(L, nm).argtypes = [vp, C.c_uint, C.c_char_p, C.c_char_p, vp, vp, dpp]
    L.nlopt_amd_device_constraint_count.argtypes = [vp]
    for nm in ("nlopt_amd_add_inequality_device_mconstraint_data", "nlopt_amd_add_equality_device_mconstraint_data"):
        getattr(L, nm).argtypes = [vp, C.c_uint, C.c_char_p, C.c_char_p, vp, vp, dpp, vp, C.c_size_t]
    L.nlopt_amd_set_device_objective_data.argtypes = [vp, vp, C.c_size_t]
    L.nlopt_amd_eval_device_objective.argtypes = [vp, C.c_size_t, dpp, dpp, dpp]
    L.nlopt_amd_set_device_objective_row_data.argtypes = [vp, C.c_size_t, C.c_size_t, vp]
    L.nlopt_amd_optimize_batch.argtypes = [vp, C.c_size_t, dpp, dpp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.nlopt_amd_local_list_launches.argtypes = [vp]
    L.nlopt_amd_local_list_launches.restype = C.c_uint64
    L.nlopt_amd_batch_constraint_launches.argtypes = [vp]
    L.nlopt_amd_batch_constraint_launches.restype = C.c_uint64
    if hasattr(L, "nla_k_local_waiting_list"):  # (not in the emulated device layer either: the host loop builds the list there)
        L.nla_k_local_waiting_list.argtypes = [vp, C.c_int, vp, vp, vp]
    if hasattr(L, "nla_k_isres_eval_cv"):       # (not in the emulated device layer: no code object loads there, so nothing needs it)
        L.nla_k_isres_eval_cv.argtypes = [C.c_int, C.c_int, C.c_int, vp, C.c_int64, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp, vp]
    L.nla_dev_malloc_uncached.argtypes = [C.c_size_t]
    L.nla_dev_malloc_uncached.restype = vp
    L.nla_dev_free_uncached.argtypes = [vp]
    L.nla_dev_free_uncached.restype = None
    L.nla_k_crs_chain.argtypes = [C.c_int, C.c_int, C.c_int, vp, C.c_int64, C.c_double, vp, vp, vp, vp, C.c_uint32, C.c_uint64, C.c_int, vp, vp,
                                  C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_uint32, vp, vp, vp, C.c_int, vp]
    L.nla_crs_chain_tickets.argtypes = [C.c_int, C.c_int, C.c_int]
    L.nla_crs_chain_tickets.restype = C.c_uint32
    L.nla_crs_chain_ctrl_bytes.argtypes = [C.c_int, C.c_int]
    L.nla_crs_chain_ctrl_bytes.restype = C.c_size_t
    L.nla_crs_chain_chunks.argtypes = [C.c_int, C.c_int]
    L.nla_k_crs_finish.argtypes = [C.c_int, C.c_int, C.c_int, vp, C.c_int64, vp, vp, vp, C.c_uint32, C.c_uint64, C.c_int,
                                   vp, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    L.nla_k_isres_rank_count.argtypes = [C.c_int64, vp, vp, vp, vp, vp]
    L.nla_k_isres_bits.argtypes = [vp, C.c_int64, C.c_int, C.c_int64, vp, vp]
    L.nla_k_isres_stochrank.argtypes = [C.c_int64, C.c_int64, vp, vp, vp, vp, vp, vp, vp]
    L.nla_k_isres_stochrank_gated.argtypes = [C.c_int64, C.c_int64, vp, vp, vp, vp, vp, vp, vp, C.c_uint64, C.c_int64, vp]   # ..., gate, gate_g_rank0, gate_nrows, stream
    L.nla_isres_evolve2_ws_bytes.restype = C.c_size_t
    L.nla_isres_evolve2_ws_bytes.argtypes = [C.c_int]
    L.nla_k_isres_inverse.argtypes = [C.c_int64, vp, vp, vp]
    L.nla_k_isres_evolve_rounds.argtypes = ([C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_double, C.c_double] + [vp] * 12 +
                                            [C.c_int, vp])   # ..., lb, ub, z, irank, inv, X, S, x0c, state, rho, ws, rounds, stream
    L.nla_k_isres_evolve.argtypes = ([C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_double, C.c_double] +
                                     [vp] * 9)   # ..., lb, ub, z, irank, X, S, scratch, state, stream
    L.nla_k_isres_evolve_parent_mu.argtypes = [C.c_int, C.c_int, C.c_int64] + [vp] * 7   # ..., lb, ub, irank, X, S, mu_rp, stream
    L.nla_isres_evolve2_supported.argtypes = [C.c_int]
    L.nla_k_crs_commit.argtypes = [C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp, vp]
    L.nla_k_crs_mutate.argtypes = [C.c_int, vp, vp, vp, vp, vp, vp]
    # the launchers crs_pass.c uses on its usual path: lists as kernel arguments (host arrays), the fused commit, the doorbell,
    # the production form of the window launch, the column-sharded pass
    L.nla_host_malloc.argtypes = [C.c_size_t]
    L.nla_host_malloc.restype = vp
    L.nla_host_free.argtypes = [vp]
    L.nla_host_free.restype = None
    L.nla_k_crs_advance_args.argtypes = L.nla_k_crs_advance.argtypes
    L.nla_k_crs_advance_cols.argtypes = [C.c_int] + L.nla_k_crs_advance.argtypes           # n, ncol, ld, ...
    L.nla_k_crs_advance_commit_args.argtypes = ([C.c_int, C.c_int, vp, C.c_int64, vp, vp, vp, C.c_uint32, C.c_uint64, C.c_int, vp, C.c_int,
                                                 vp, vp, C.c_int, vp, vp, vp] +
                                                [vp, C.c_int, vp, vp, vp, C.c_int, vp])   # ..., TX, TM, ncommit, h_slot, h_kind, h_row, variant, stream
    L.nla_k_crs_finish_args.argtypes = L.nla_k_crs_finish.argtypes
    L.nla_k_crs_finish_args_bell.argtypes = L.nla_k_crs_finish.argtypes[:-1] + [vp, vp, C.c_uint32, vp]   # ..., status, bell_count, bell, bell_seq, stream
    L.nla_k_crs_commit_args.argtypes = L.nla_k_crs_commit.argtypes
    L.nla_k_crs_commit_zero.argtypes = L.nla_k_crs_commit.argtypes[:-1] + [C.c_int, vp, C.c_size_t, vp]   # ..., row, lists_on_host, zero, zero_bytes, stream
    L.nla_k_crs_chain_lean.argtypes = L.nla_k_crs_chain.argtypes[:-1] + [C.c_int, vp]                      # ..., fwcap, ctrl_is_zero, stream
    L.nla_k_crs_sh_init_rows.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int64, C.c_int64, vp, vp]
    L.nla_k_crs_sh_mutate_pack.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int64, vp, vp, vp, C.c_uint32, C.c_uint64, C.c_int,
                                           vp, vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, vp]
    L.nla_k_crs_sh_eval.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int, vp, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp]
    L.nla_k_crs_commit_sh.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp, vp, C.c_size_t,
                                      C.c_int, C.c_int, C.c_int, vp, vp]
    L.nla_mt_jump_poly_words.argtypes = [C.c_uint64, vp]
    L.nla_mt_jump_poly_words.restype = None
    L.nla_mt_jump_poly_pow2.argtypes = [C.c_int]
    L.nla_mt_jump_poly_pow2.restype = vp
    L.nla_mt_apply_jump_host.argtypes = [vp, vp, vp]
    L.nla_mt_apply_jump_host.restype = None
    L.nla_mt_advance_blocks_host.argtypes = [vp, C.c_uint64, vp]
    L.nla_mt_advance_blocks_host.restype = None
    L.nla_mt_export.argtypes = [vp, C.POINTER(C.c_int)]
    L.nla_mt_export.restype = None
    L.nla_mt_import.argtypes = [vp, C.c_int]
    L.nla_mt_import.restype = None
    L.nla_mt_charpoly_terms.argtypes = [C.POINTER(C.POINTER(C.c_int))]
    # multi-GPU collectives (comm.c)
    L.nlopt_amd_rccl_unique_id.argtypes = [vp]
    L.nlopt_amd_comm_create_rccl.argtypes = [C.c_int, C.c_int, vp]
    L.nlopt_amd_comm_create_rccl.restype = vp
    L.nlopt_amd_comm_create_host.argtypes = [C.c_int, C.c_int, vp, vp]
    L.nlopt_amd_comm_create_host.restype = vp
    L.nlopt_amd_comm_destroy.argtypes = [vp]
    L.nlopt_amd_comm_destroy.restype = None
    L.nlopt_amd_comm_rank.argtypes = [vp]
    L.nlopt_amd_comm_world.argtypes = [vp]
    L.nlopt_amd_comm_error.argtypes = [vp]
    L.nlopt_amd_comm_error.restype = C.c_char_p
    L.nlopt_amd_comm_counters.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.nlopt_amd_comm_counters.restype = None
    L.nlopt_amd_set_comm.argtypes = [vp, vp]
    L.nlopt_amd_set_progress.argtypes = [vp, vp, vp]
    L.nla_comm_allgather_host.argtypes = [vp, vp, vp, C.c_size_t, vp]
    L.nla_comm_allgather_dev.argtypes = [vp, vp, vp, C.c_size_t, vp]
    L.nla_comm_partition.argtypes = [vp, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.nla_comm_partition.restype = None
    L.nla_dev_set.argtypes = [C.c_int]
    _lib = L
    return L


def device_count():
    return lib().nlopt_amd_device_count()


def srand(seed):
    lib().nlopt_srand(seed)


def objective(name_or_id):
    """the registered host callback for a device objective (pass it to set_min_objective)"""
    i = OBJECTIVES[name_or_id] if isinstance(name_or_id, str) else int(name_or_id)
    return lib().nlopt_amd_objective(i)


def objective_box(name_or_id):
    i = OBJECTIVES[name_or_id] if isinstance(name_or_id, str) else int(name_or_id)
    lo, hi = C.c_double(), C.c_double()
    lib().nlopt_amd_objective_box(i, C.byref(lo), C.byref(hi))
    return lo.value, hi.value


class DevBuf:
    """a device allocation owned by libnlopt_amd's runtime layer, with numpy staging"""

    def __init__(self, nbytes, uncached=False):
        self.nbytes = int(nbytes)
        self.uncached = bool(uncached)
        self.ptr = (lib().nla_dev_malloc_uncached if uncached else lib().nla_dev_malloc)(self.nbytes)
        if not self.ptr:
            raise MemoryError("nla_dev_malloc(%d) failed" % self.nbytes)

    @classmethod
    def from_array(cls, a, uncached=False):
        a = np.ascontiguousarray(a)
        b = cls(max(a.nbytes, 1), uncached)
        L = lib()
        rc = L.nla_memcpy_h2d(b.ptr, a.ctypes.data, a.nbytes, None) or L.nla_stream_sync(None)
        if rc:
            raise RuntimeError("H2D failed: %s" % L.nla_dev_error_string(rc))
        return b

    def to_array(self, dtype, count):
        out = np.empty(count, dtype=dtype)
        L = lib()
        rc = L.nla_memcpy_d2h(out.ctypes.data, self.ptr, out.nbytes, None) or L.nla_stream_sync(None)
        if rc:
            raise RuntimeError("D2H failed: %s" % L.nla_dev_error_string(rc))
        return out

    def free(self):
        if self.ptr:
            (lib().nla_dev_free_uncached if getattr(self, "uncached", False) else lib().nla_dev_free)(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


PROGRESS_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_long, C.c_long)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)


class Comm:
    """The communicator of a multi-GPU run (include/nlopt_amd.h, comm.c): one process per GPU, every rank
    builds the same Opt, calls srand() with the same seed and optimize() with the same arguments."""

    def __init__(self, handle, keep=None):
        self._L = lib()
        self._h = handle
        self._keep = keep
        if not handle:
            raise RuntimeError("could not create the communicator")

    @classmethod
    def rccl(cls, rank, world, uid):
        """RCCL over xGMI; `uid` = the 128 bytes of rccl_unique_id() made on rank 0. Call after selecting the device."""
        buf = C.create_string_buffer(bytes(uid), 128)
        return cls(lib().nlopt_amd_comm_create_rccl(int(rank), int(world), C.cast(buf, C.c_void_p)))

    @classmethod
    def shm(cls, rank, world, name, slot_bytes=0):
        """ranks on one node over a POSIX shared-memory segment (comm.c: copy in, one barrier, copy out; device data go straight
        into / out of the registered slots).  `name`: "/..." — the same on every rank, unique to the job."""
        L = lib()
        L.nlopt_amd_comm_create_shm.restype = C.c_void_p
        L.nlopt_amd_comm_create_shm.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_size_t]
        return cls(L.nlopt_amd_comm_create_shm(int(rank), int(world), name.encode(), int(slot_bytes)))

    @classmethod
    def host(cls, rank, world, allgather):
        """host transport: allgather(send: bytes) -> bytes of length world*len(send), rank-major"""
        def _cb(ctx, send, recv, nbytes):
            try:
                out = allgather(C.string_at(send, nbytes))
                if len(out) != nbytes * world:
                    return 2
                C.memmove(recv, out, len(out))
                return 0
            except Exception:           # must not propagate through the C frames
                import traceback
                traceback.print_exc()
                return 1
        fn = ALLGATHER_FN(_cb)
        return cls(lib().nlopt_amd_comm_create_host(int(rank), int(world), C.cast(fn, C.c_void_p), None), keep=fn)

    @classmethod
    def from_torch_distributed(cls, group=None):
        """communicator over an initialised torch.distributed process group: backend nccl (= RCCL on ROCm)
        -> the library's own RCCL communicator (the unique id is broadcast through the group); gloo ->
        host transport through dist.all_gather_into_tensor on CPU tensors."""
        import torch
        import torch.distributed as dist
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        # (NLA_RCCL_LIBRARY: the library's RCCL transport whatever the group's backend — the group only carries the unique id;
        # the tests bind a contract-checking stand-in for librccl that way, a site its own RCCL build)
        if dist.get_backend(group) == "nccl" or os.environ.get("NLA_RCCL_LIBRARY"):
            uid = [rccl_unique_id() if rank == 0 else None]
            dist.broadcast_object_list(uid, src=0, group=group)
            return cls.rccl(rank, world, uid[0])

        def allgather(b):
            t = torch.frombuffer(bytearray(b), dtype=torch.uint8)
            out = torch.empty(world * t.numel(), dtype=torch.uint8)
            dist.all_gather_into_tensor(out, t, group=group)
            return out.numpy().tobytes()
        return cls.host(rank, world, allgather)

    @property
    def rank(self): return self._L.nlopt_amd_comm_rank(self._h)

    @property
    def world(self): return self._L.nlopt_amd_comm_world(self._h)

    def counters(self):
        a, b = C.c_uint64(), C.c_uint64()
        self._L.nlopt_amd_comm_counters(self._h, C.byref(a), C.byref(b))
        return dict(collectives=a.value, bytes=b.value)

    def error(self):
        return self._L.nlopt_amd_comm_error(self._h).decode()

    def allgather_host(self, a):
        """all-gather of a numpy array over the communicator's host path (tests)"""
        a = np.ascontiguousarray(a)
        out = np.empty((self.world,) + a.shape, dtype=a.dtype)
        rc = self._L.nla_comm_allgather_host(self._h, a.ctypes.data, out.ctypes.data, a.nbytes, None)
        if rc:
            raise RuntimeError("all-gather failed: " + self.error())
        return out

    def partition(self, count):
        per, first, mine = C.c_int64(), C.c_int64(), C.c_int64()
        self._L.nla_comm_partition(self._h, count, C.byref(per), C.byref(first), C.byref(mine))
        return per.value, first.value, mine.value

    def destroy(self):
        h, self._h = self._h, None
        if h:
            self._L.nlopt_amd_comm_destroy(h)


def rccl_unique_id():
    buf = C.create_string_buffer(128)
    if lib().nlopt_amd_rccl_unique_id(C.cast(buf, C.c_void_p)) != 0:
        raise RuntimeError("RCCL is not available (librccl.so could not be loaded)")
    return buf.raw


def _data_bytes(data):
    """a data block for a device objective / constraint block as bytes (None stays None: no data)"""
    if data is None:
        return None
    if isinstance(data, (bytes, bytearray, memoryview)):
        return bytes(data)
    return np.ascontiguousarray(data).tobytes()


class Opt:
    """Mirror of the reference's `nlopt.opt` Python class over the C API (subset used by the hot path)."""

    def __init__(self, algorithm, n):
        self._L = lib()
        self._h = self._L.nlopt_create(int(algorithm), int(n))
        if not self._h:
            raise ValueError("nlopt_create failed (bad algorithm?)")
        self.n = int(n)
        self._keep = []
        self._trace = None
        self._last = None
        self._minf = None

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._L.nlopt_destroy(h)

    def copy(self):
        """nlopt_copy: an independent Opt with the same settings; a bound device objective's kernel and data block are shared
        (reference counted), and the Python callbacks this object keeps alive stay alive with the copy"""
        h = self._L.nlopt_copy(self._h)
        if not h:
            raise MemoryError("nlopt_copy failed")
        c = Opt.__new__(Opt)
        c._L, c._h, c.n, c._keep, c._trace, c._last, c._minf = self._L, h, self.n, list(self._keep), None, None, None
        return c

    def _ck(self, ret):
        if ret < 0:
            msg = self._L.nlopt_get_errmsg(self._h)
            raise RuntimeError("nlopt error %d (%s)%s" % (ret, self._L.nlopt_result_to_string(ret).decode(),
                                                          ": " + msg.decode() if msg else ""))
        return ret

    # -- objective / bounds / constraints --
    def _fptr(self, f):
        if isinstance(f, int):
            return f
        cb = NLOPT_FUNC(lambda n, x, g, d: float(f(np.ctypeslib.as_array(x, shape=(n,)),
                                                    np.ctypeslib.as_array(g, shape=(n,)) if g else np.empty(0))))
        self._keep.append(cb)
        return C.cast(cb, C.c_void_p).value

    def set_min_objective(self, f, f_data=None):
        self._ck(self._L.nlopt_set_min_objective(self._h, self._fptr(f), f_data))

    def set_max_objective(self, f, f_data=None):
        self._ck(self._L.nlopt_set_max_objective(self._h, self._fptr(f), f_data))

    def set_min_device_objective(self, code_object, name, host_twin=None, maximize=False):
        """bind a user-supplied device objective (include/nlopt_amd_device.h): kernel <name>_evalgrad of the code object"""
        fn = self._L.nlopt_amd_set_max_device_objective if maximize else self._L.nlopt_amd_set_min_device_objective
        fn.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_void_p, C.c_void_p]
        return fn(self._h, code_object.encode(), name.encode(), self._fptr(host_twin) if host_twin is not None else None, None)

    def set_device_objective_data(self, data):
        """the data the bound ABI-2 device objective reads (NLOPT_AMD_DEVICE_OBJECTIVE_DATA / _RESIDUALS of nlopt_amd_device.h): a numpy
        array or bytes, copied to the device at the call; None or empty clears it.  Belongs to this Opt: a copy shares it until either
        side sets data again."""
        buf = _data_bytes(data)
        return self._L.nlopt_amd_set_device_objective_data(self._h, buf, len(buf) if buf is not None else 0)

    def set_device_objective_row_data(self, rows):
        """the data rows the bound ABI-3 device objective reads (NLOPT_AMD_DEVICE_OBJECTIVE_ROWS / _RESIDUALS_ROWS of nlopt_amd_device.h):
        a 2-d array, one row per search of optimize_batch (search i reads row i), copied to the device at the call; None or an array
        without rows clears it"""
        if rows is None:
            return self._L.nlopt_amd_set_device_objective_row_data(self._h, 0, 0, None)
        a = np.ascontiguousarray(rows)
        if a.ndim != 2:
            raise ValueError("set_device_objective_row_data takes a 2-d array: one row per search")
        return self._L.nlopt_amd_set_device_objective_row_data(self._h, a.shape[0], a.shape[1] * a.itemsize, a.ctypes.data)

    def eval_device_objective(self, X, grad=False):
        """f (and, grad=True, the gradient) of the bound device objective at the rows of X, one launch of the user's kernel: f of shape
        (count,), or (f, G) with G of shape (count, n).  A single point (shape (n,)) gives a float, or (float, g)."""
        X = np.ascontiguousarray(X, dtype=np.float64)
        single = X.ndim == 1
        X = X.reshape(-1, self.n)
        f = np.empty(X.shape[0])
        G = np.empty_like(X) if grad else None
        self._ck(self._L.nlopt_amd_eval_device_objective(self._h, X.shape[0], _dp(X), _dp(f), _dp(G) if grad else None))
        if single:
            return (float(f[0]), G[0]) if grad else float(f[0])
        return (f, G) if grad else f

    def set_lower_bounds(self, lb):
        if np.isscalar(lb):
            self._ck(self._L.nlopt_set_lower_bounds1(self._h, float(lb)))
        else:
            self._ck(self._L.nlopt_set_lower_bounds(self._h, _dp(np.ascontiguousarray(lb, dtype=np.float64))))

    def set_upper_bounds(self, ub):
        if np.isscalar(ub):
            self._ck(self._L.nlopt_set_upper_bounds1(self._h, float(ub)))
        else:
            self._ck(self._L.nlopt_set_upper_bounds(self._h, _dp(np.ascontiguousarray(ub, dtype=np.float64))))

    def get_lower_bounds(self):
        a = np.empty(self.n)
        self._ck(self._L.nlopt_get_lower_bounds(self._h, _dp(a)))
        return a

    def get_upper_bounds(self):
        a = np.empty(self.n)
        self._ck(self._L.nlopt_get_upper_bounds(self._h, _dp(a)))
        return a

    def add_inequality_constraint(self, fc, tol=0.0, f_data=None):
        return self._L.nlopt_add_inequality_constraint(self._h, self._fptr(fc), f_data, float(tol))

    def add_equality_constraint(self, h, tol=0.0, f_data=None):
        return self._L.nlopt_add_equality_constraint(self._h, self._fptr(h), f_data, float(tol))

    def add_blocksum_constraints(self, count, tol=1e-8, equality=False):
        """`count` device constraints g_q(x) = sum_{i in block q of `count`} x_i - 1 (<= 0, or == 0)"""
        data = (C.c_uint * (2 * max(count, 1)))()
        self._keep.append(data)
        cb = C.cast(self._L.nlopt_amd_constraint_blocksum(), C.c_void_p).value
        add = self._L.nlopt_add_equality_constraint if equality else self._L.nlopt_add_inequality_constraint
        for q in range(count):
            data[2 * q], data[2 * q + 1] = q, count
            self._ck(add(self._h, cb, C.addressof(data) + 8 * q, float(tol)))

    def _add_device_constraints(self, equality, code_object, name, m, host_twin, tol, data=None):
        fn = self._L.nlopt_amd_add_equality_device_mconstraint if equality else self._L.nlopt_amd_add_inequality_device_mconstraint
        if data is not None:
            fn = self._L.nlopt_amd_add_equality_device_mconstraint_data if equality else self._L.nlopt_amd_add_inequality_device_mconstraint_data
        twin = None
        if host_twin is not None:
            def _cb(mm, res, n, x, g, d):
                v = host_twin(np.ctypeslib.as_array(x, shape=(n,)))
                for j in range(mm):
                    res[j] = float(v[j])
            cb = NLOPT_MFUNC(_cb)
            self._keep.append(cb)
            twin = C.cast(cb, C.c_void_p).value
        t = None
        if tol is not None:
            t = np.ascontiguousarray(np.broadcast_to(np.asarray(tol, dtype=np.float64), (int(m),)))
        args = (self._h, int(m), code_object.encode() if code_object is not None else None, name.encode() if name is not None else None,
                twin, None, _dp(t) if t is not None else None)
        if data is not None:
            buf = _data_bytes(data)
            return fn(*args, buf, len(buf))
        return fn(*args)

    def add_inequality_device_constraints(self, code_object, name, m, host_twin=None, tol=None, data=None):
        """bind a block of m user-supplied device constraints g_j(x) <= 0 (include/nlopt_amd_device.h): kernel <name>_coneval of the
        code object; host_twin(x) -> sequence of m values is what the host paths call; tol: scalar or m tolerances (None: zeros);
        data (numpy array or bytes): what an ABI-2 block (NLOPT_AMD_DEVICE_CONSTRAINTS_DATA, kernel <name>_coneval_d) reads, copied
        to the device at the call.  NLOPT_GN_ISRES evaluates the block for a whole population per launch; optimize_batch with
        LN_COBYLA (a user device objective, every constraint a bound block) evaluates it for all searches of a chunk per step; every
        other path sees host_twin, or single points through the kernel"""
        return self._add_device_constraints(False, code_object, name, m, host_twin, tol, data)

    def add_equality_device_constraints(self, code_object, name, m, host_twin=None, tol=None, data=None):
        """... the same as equality constraints h_j(x) == 0"""
        return self._add_device_constraints(True, code_object, name, m, host_twin, tol, data)

    def batch_constraint_launches(self):
        """the last optimize_batch of this optimiser: launches of bound constraint blocks (one per block and coroutine step of a chunk;
        0 for an unconstrained batch)"""
        return self._L.nlopt_amd_batch_constraint_launches(self._h)

    def device_constraint_count(self):
        return self._L.nlopt_amd_device_constraint_count(self._h)

    # -- stopping criteria & parameters --
    def set_stopval(self, v): self._ck(self._L.nlopt_set_stopval(self._h, float(v)))
    def set_ftol_rel(self, v): self._ck(self._L.nlopt_set_ftol_rel(self._h, float(v)))
    def set_ftol_abs(self, v): self._ck(self._L.nlopt_set_ftol_abs(self._h, float(v)))
    def set_xtol_rel(self, v): self._ck(self._L.nlopt_set_xtol_rel(self._h, float(v)))
    def set_xtol_abs(self, v):
        if np.isscalar(v):
            self._ck(self._L.nlopt_set_xtol_abs1(self._h, float(v)))
        else:
            self._ck(self._L.nlopt_set_xtol_abs(self._h, _dp(np.ascontiguousarray(v, dtype=np.float64))))
    def set_maxeval(self, v): self._ck(self._L.nlopt_set_maxeval(self._h, int(v)))
    def set_maxtime(self, v): self._ck(self._L.nlopt_set_maxtime(self._h, float(v)))
    def set_population(self, v): self._ck(self._L.nlopt_set_population(self._h, int(v)))

    def set_progress(self, fn):
        """fn(generations_done, numevals) at the start of every ISRES generation / MLSL iteration"""
        cb = PROGRESS_FN(lambda d, g, e: fn(g, e)) if fn else None
        self._progress = cb
        self._ck(self._L.nlopt_amd_set_progress(self._h, C.cast(cb, C.c_void_p) if cb else None, None))

    def set_comm(self, comm):
        """multi-GPU run over `comm` (a Comm, kept alive by this object); None = single process"""
        self._comm = comm
        self._ck(self._L.nlopt_amd_set_comm(self._h, comm._h if comm is not None else None))

    def set_param(self, name, v): self._ck(self._L.nlopt_set_param(self._h, name.encode(), float(v)))
    def get_numevals(self): return self._L.nlopt_get_numevals(self._h)
    def get_errmsg(self):
        m = self._L.nlopt_get_errmsg(self._h)
        return m.decode() if m else None
    def force_stop(self): self._L.nlopt_force_stop(self._h)

    # -- libnlopt_amd additions --
    def enable_trace(self, cap):
        self._trace = np.zeros(int(cap), dtype=TRACE_DTYPE)
        self._L.nlopt_amd_set_trace(self._h, self._trace.ctypes.data, int(cap))

    def trace(self):
        k = min(self._L.nlopt_amd_trace_len(self._h), len(self._trace))
        return self._trace[:k].copy()

    def trace_len(self):
        return self._L.nlopt_amd_trace_len(self._h)

    def stats(self):
        s = Stats()
        self._L.nlopt_amd_get_stats(self._h, C.byref(s))
        d = s.asdict()
        d["local_list_launches"] = self._L.nlopt_amd_local_list_launches(self._h)     # (a counter of its own beside nlopt_amd_stats)
        return d

    # -- run --
    def optimize_raw(self, x0):
        """returns (x, minf, nlopt_result) without raising on negative results"""
        x = np.array(x0, dtype=np.float64)
        minf = C.c_double()
        ret = self._L.nlopt_optimize(self._h, _dp(x), C.byref(minf))
        self._last, self._minf = ret, minf.value
        return x, minf.value, ret

    def optimize_batch(self, X0):
        """nlopt_amd_optimize_batch: one local search (LD_LBFGS, LD_MMA, LN_COBYLA, LN_NELDERMEAD, LN_SBPLX, LD_TNEWTON*) from every row of X0, side by side on the device.
        Nonlinear constraints are served for LN_COBYLA on a user device objective when every one of them is a bound device block
        (add_inequality_device_constraints / add_equality_device_constraints); anything else with constraints is refused.
        Returns (X, minf, results, numevals): the minimisers (count, n) and per search its value, nlopt_result and evaluation count.
        The call's own result is in last_optimize_result(); a negative one other than FORCED_STOP raises."""
        X = np.array(X0, dtype=np.float64).reshape(-1, self.n)
        count = X.shape[0]
        minf = np.full(count, np.nan)
        results = np.zeros(count, dtype=np.intc)
        nev = np.zeros(count, dtype=np.intc)
        ret = self._L.nlopt_amd_optimize_batch(self._h, count, _dp(X), _dp(minf), results.ctypes.data_as(C.POINTER(C.c_int)),
                                               nev.ctypes.data_as(C.POINTER(C.c_int)))
        self._last, self._minf = ret, None
        if ret != FORCED_STOP:
            self._ck(ret)
        return X, minf, results, nev

    def optimize(self, x0):
        x, _, ret = self.optimize_raw(x0)
        self._ck(ret)
        return x

    def last_optimum_value(self): return self._minf
    def last_optimize_result(self): return self._last
