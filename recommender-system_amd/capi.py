"""ctypes bindings of the two in-tree libraries -- the same stubs INTEGRATION.md shows for the reference.

  csrc/libmatfact_hip.so   include/matfact_hip.h   (HIP kernels, C ABI; replaces matFact.c:29 / :10 / mat2d.c:100)
  host/libmatfact_host.so  include/matfact_host.h  (parser, init, partition, synthetic generator)

Loading is strict: a missing library raises ImportError; nothing here computes on the CPU in its place.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# MF_HIP_LIB: alternative build of the same library (A/B timing of kernel variants); never a different backend
HIP_LIB_PATH = os.environ.get("MF_HIP_LIB") or os.path.join(_HERE, "csrc", "libmatfact_hip.so")
HOST_LIB_PATH = os.path.join(_HERE, "host", "libmatfact_host.so")
CLI_PATH = os.path.join(_HERE, "host", "matFact")

_i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_i64p = np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")
_f64p = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")

MF_OK = 0
MF_ERR_ARGUMENT, MF_ERR_NO_DEVICE, MF_ERR_HIP, MF_ERR_NO_MEMORY, MF_ERR_UNSUPPORTED, MF_ERR_STATE = -1, -2, -3, -4, -5, -6
MF_TOPN_MAX = 32
MF_LOSS_BLOCK = 1024
MF_LOSS_TRAIN, MF_LOSS_HELDOUT = 0, 1
MF_RANK_MASKED, MF_RANK_NAN = -1, -2
MF_SIMILAR_DOT, MF_SIMILAR_COSINE = 0, 1
SIMILAR_METRICS = {"dot": MF_SIMILAR_DOT, "cosine": MF_SIMILAR_COSINE}

# every symbol include/matfact_hip.h declares (tests check the library exports each one)
HIP_SYMBOLS = [
    "mf_backend_strerror", "mf_backend_last_hip_error", "mf_backend_abi_version", "mf_backend_device_count",
    "mf_backend_factorize", "mf_backend_recommend", "mf_backend_run", "mf_backend_run_multi", "mf_backend_run_top1",
    "mf_backend_multi_last_timing", "mf_backend_multi_last_counters",
    "mf_plan_create", "mf_backend_row_pitch", "mf_plan_row_pitch", "mf_plan_destroy", "mf_plan_set_stream", "mf_plan_upload_factors",
    "mf_plan_download_factors", "mf_plan_iterate", "mf_plan_sweep_items", "mf_plan_sweep_users",
    "mf_plan_items_next", "mf_plan_items_current", "mf_plan_flip", "mf_plan_recommend", "mf_plan_recommend_info",
    "mf_plan_sweep_users_seeded", "mf_plan_users_next", "mf_plan_users_current", "mf_plan_recommend_scored",
    "mf_plan_recommend_scored_users", "mf_plan_recommend_filter", "mf_backend_recommend_margin",
    "mf_plan_predict", "mf_plan_synchronize",
    "mf_plan_timing", "mf_plan_timing_read", "mf_plan_describe",
    "mf_backend_recommend_topn", "mf_backend_run_topn", "mf_plan_recommend_topn", "mf_plan_recommend_topn_info",
    "mf_plan_set_heldout", "mf_plan_loss", "mf_backend_loss_total", "mf_plan_iterate_monitored", "mf_backend_loss",
    "mf_plan_rank_heldout", "mf_plan_rank_heldout_info", "mf_backend_rank_metrics",
    "mf_plan_similar_items", "mf_plan_similar_items_info", "mf_backend_similar_items",
    "mf_plan_set_regularization", "mf_plan_get_regularization", "mf_plan_penalty", "mf_backend_run_reg",
    "mf_plan_set_frozen_columns", "mf_plan_get_frozen_columns", "mf_backend_bias_mean", "mf_backend_bias_pack",
    "mf_backend_bias_unpack", "mf_backend_run_biased",
    "mf_plan_set_momentum", "mf_plan_get_momentum", "mf_plan_upload_previous", "mf_plan_download_previous",
    "mf_backend_run_momentum",
    "mf_plan_create_weighted", "mf_plan_weight_total", "mf_backend_run_weighted",
    "mf_plan_set_bounds", "mf_plan_get_bounds", "mf_plan_project", "mf_plan_bounds_active", "mf_backend_run_bounded",
    "mf_plan_set_adaptive", "mf_plan_get_adaptive", "mf_plan_reset_adaptive", "mf_plan_adaptive_finish",
    "mf_plan_download_adaptive_state", "mf_plan_upload_adaptive_state", "mf_backend_run_adaptive",
    "mf_plan_set_als", "mf_plan_get_als", "mf_plan_als_solve", "mf_plan_als_info", "mf_backend_run_als",
    "mf_plan_gram", "mf_plan_set_confidence", "mf_plan_get_confidence", "mf_plan_implicit_objective", "mf_backend_gram_dot",
    "mf_backend_run_implicit",
    "mf_plan_set_als_cg", "mf_plan_get_als_cg", "mf_backend_run_als_cg",
    "mf_plan_set_implicit_cg", "mf_plan_get_implicit_cg", "mf_backend_run_implicit_cg",
    "mf_backend_als_normal_pitch", "mf_plan_als_normal", "mf_plan_als_solve_normal",
    "mf_plan_set_als_box", "mf_plan_get_als_box", "mf_backend_run_als_box",
]
HOST_SYMBOLS = [
    "mf_host_parse_strerror", "mf_host_parse_file", "mf_host_parse_buffer", "mf_host_free_problem",
    "mf_host_parse_file_cached",
    "mf_host_srandom", "mf_host_random", "mf_host_init_factors", "mf_host_init_factors_block",
    "mf_host_split_entries", "mf_host_partition_users", "mf_host_balanced_grid", "mf_host_write_out", "mf_host_checkpoint_write",
    "mf_host_checkpoint_read", "mf_host_synth_counts",
    "mf_host_synth_fill", "mf_host_write_topn",
]


class HipBackendError(RuntimeError):
    def __init__(self, status, where):
        self.status = status
        msg = hip().mf_backend_strerror(status).decode()
        detail = hip().mf_backend_last_hip_error().decode() if status == MF_ERR_HIP else ""
        super().__init__("%s: %s (%d) %s" % (where, msg, status, detail))


class Entry(C.Structure):  # mf_entry == non_zero_entry (datatypes.h:10-15)
    _fields_ = [("row", C.c_int32), ("col", C.c_int32), ("value", C.c_double)]


class Problem(C.Structure):  # mf_problem
    _fields_ = [("users", C.c_int32), ("items", C.c_int32), ("features", C.c_int32), ("iters", C.c_int32),
                ("alpha", C.c_double), ("nnz", C.c_int64), ("entries", C.POINTER(Entry))]


class Shard(C.Structure):  # mf_shard
    _fields_ = [("users_total", C.c_int32), ("items", C.c_int32), ("features", C.c_int32),
                ("user_begin", C.c_int32), ("user_count", C.c_int32), ("nnz", C.c_int64),
                ("row", C.c_void_p), ("col", C.c_void_p), ("val", C.c_void_p), ("alpha", C.c_double),
                ("device", C.c_int32), ("flags", C.c_int32), ("items_ext", C.c_void_p * 2),
                ("users_ext", C.c_void_p * 2), ("items_pitch", C.c_int32), ("users_pitch", C.c_int32)]


# mf_candidate: the partial scan state of mf_plan_recommend_scored, as a numpy record layout
# mf_filter: pass-1 (matrix-core) report of mf_plan_recommend_filter
FILTER_DTYPE = np.dtype([("best", np.float64), ("second", np.float64), ("arg", np.int32), ("nonfinite", np.int32)])
CANDIDATE_DTYPE = np.dtype([("score", np.float64), ("best", np.int32), ("first", np.int32),
                            ("first_nan", np.int32), ("reserved", np.int32)])


class Bounds(C.Structure):  # mf_bounds
    _fields_ = [("lo", C.c_double), ("hi", C.c_double), ("columns", C.c_int32)]


class Adaptive(C.Structure):  # mf_adaptive
    _fields_ = [("kind", C.c_int32), ("eta", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double)]


# MF_OPT_*: the kinds of an adaptive rule, by number and by name
MF_OPT_NONE, MF_OPT_ADAGRAD, MF_OPT_RMSPROP, MF_OPT_ADAM = 0, 1, 2, 3
OPTIMIZERS = {"none": 0, "adagrad": 1, "rmsprop": 2, "adam": 3, None: 0, 0: 0, 1: 1, 2: 2, 3: 3}
OPTIMIZER_NAMES = ("none", "adagrad", "rmsprop", "adam")

# MF_ALS_*: the kinds of the ALS solver, by number and by name
MF_ALS_OFF, MF_ALS_RIDGE, MF_ALS_RIDGE_COUNT = 0, 1, 2
MF_ALS_IMPLICIT = 4   # 3 is not a kind
ALS_KINDS = {"off": 0, "ridge": 1, "ridge-count": 2, "implicit": 4, None: 0, 0: 0, 1: 1, 2: 2, 4: 4}
ALS_KIND_NAMES = ("off", "ridge", "ridge-count", None, "implicit")


class ImplicitObjective(C.Structure):  # mf_implicit_objective
    _fields_ = [("all_sq", C.c_double), ("observed", C.c_double), ("count", C.c_int64)]


class Loss(C.Structure):  # mf_loss
    _fields_ = [("sse", C.c_double), ("count", C.c_int64)]

    @property
    def rmse(self):
        return float(np.sqrt(self.sse / self.count)) if self.count > 0 else float("nan")


class LossPoint(C.Structure):  # mf_loss_point
    _fields_ = [("iter", C.c_int32), ("reserved", C.c_int32), ("train", Loss), ("heldout", Loss)]


class RankMetrics(C.Structure):  # mf_rank_metrics
    _fields_ = [("evaluated", C.c_int64), ("masked", C.c_int64), ("nan", C.c_int64), ("users", C.c_int64),
                ("hits", C.c_int64), ("hit_rate", C.c_double), ("mrr", C.c_double), ("ndcg", C.c_double)]


class Synth(C.Structure):  # mf_synth
    _fields_ = [("seed", C.c_uint64), ("users", C.c_int32), ("items", C.c_int32), ("min_row", C.c_int32),
                ("max_row", C.c_int32), ("mode", C.c_int32), ("reserved", C.c_int32), ("target_nnz", C.c_int64)]


SYNTH_MODES = {"stratified": 0, "uniform": 1, "zipf": 2}


class Rand(C.Structure):  # mf_rand
    _fields_ = [("ring", C.c_int32 * 31), ("f", C.c_int), ("b", C.c_int)]


_hip = None
_host = None


def hip():
    """The HIP backend library.  Raises ImportError when it has not been built (no fallback)."""
    global _hip
    if _hip is None:
        if not os.path.exists(HIP_LIB_PATH):
            raise ImportError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950); there is no CPU fallback" % HIP_LIB_PATH)
        lib = C.CDLL(HIP_LIB_PATH)
        P = C.c_void_p
        lib.mf_backend_strerror.restype = C.c_char_p
        lib.mf_backend_strerror.argtypes = [C.c_int]
        lib.mf_backend_last_hip_error.restype = C.c_char_p
        lib.mf_backend_run.argtypes = [C.POINTER(Problem), _f64p, _f64p, _i32p, C.c_int]
        lib.mf_backend_run_multi.argtypes = [C.POINTER(Problem), _f64p, _f64p, _i32p, _i32p, C.c_int]
        lib.mf_backend_multi_last_timing.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                     C.POINTER(C.c_double), C.POINTER(C.c_int * 3)]
        lib.mf_backend_multi_last_counters.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int)]
        lib.mf_backend_run_top1.argtypes = [C.POINTER(Problem), _f64p, _f64p, _i32p, C.c_int]
        lib.mf_backend_factorize.argtypes = [C.POINTER(Problem), _f64p, _f64p, C.c_int]
        lib.mf_backend_recommend.argtypes = [C.POINTER(Problem), _f64p, _f64p, _i32p, C.c_int]
        lib.mf_plan_create.argtypes = [C.POINTER(P), C.POINTER(Shard)]
        lib.mf_backend_row_pitch.argtypes = [C.c_int]
        lib.mf_plan_row_pitch.argtypes = [P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        lib.mf_plan_destroy.argtypes = [P]
        lib.mf_plan_destroy.restype = None
        lib.mf_plan_set_stream.argtypes = [P, P]
        lib.mf_plan_upload_factors.argtypes = [P, P, P]
        lib.mf_plan_download_factors.argtypes = [P, P, P]
        lib.mf_plan_iterate.argtypes = [P, C.c_int]
        lib.mf_plan_sweep_items.argtypes = [P, C.c_int]
        lib.mf_plan_sweep_users.argtypes = [P]
        lib.mf_plan_items_next.argtypes = [P]
        lib.mf_plan_items_next.restype = P
        lib.mf_plan_items_current.argtypes = [P]
        lib.mf_plan_items_current.restype = P
        lib.mf_plan_flip.argtypes = [P]
        lib.mf_plan_sweep_users_seeded.argtypes = [P, C.c_int]
        lib.mf_plan_users_next.argtypes = [P]
        lib.mf_plan_users_next.restype = P
        lib.mf_plan_users_current.argtypes = [P]
        lib.mf_plan_users_current.restype = P
        lib.mf_plan_recommend_scored.argtypes = [P, P]
        lib.mf_plan_recommend_scored_users.argtypes = [P, _i32p, C.c_int32, P]
        lib.mf_plan_recommend_filter.argtypes = [P, P, _f64p, C.POINTER(C.c_double)]
        lib.mf_backend_recommend_margin.argtypes = [C.c_int]
        lib.mf_backend_recommend_margin.restype = C.c_double
        lib.mf_plan_recommend.argtypes = [P, _i32p]
        lib.mf_plan_recommend_info.argtypes = [P, C.POINTER(C.c_int64)]
        lib.mf_plan_predict.argtypes = [P, _f64p]
        lib.mf_plan_synchronize.argtypes = [P]
        lib.mf_plan_timing.argtypes = [P, C.c_int]
        lib.mf_plan_timing_read.argtypes = [P, C.POINTER(C.c_int64), C.POINTER(C.c_double),
                                            C.POINTER(C.c_int64), C.POINTER(C.c_double)]
        lib.mf_plan_describe.argtypes = [P, C.c_char_p, C.c_int]
        lib.mf_backend_recommend_topn.argtypes = [C.POINTER(Problem), P, P, C.c_int32, P, P, C.c_int]
        lib.mf_backend_run_topn.argtypes = [C.POINTER(Problem), P, P, C.c_int32, P, P, C.c_int]
        lib.mf_plan_recommend_topn.argtypes = [P, C.c_int32, P, P]
        lib.mf_plan_recommend_topn_info.argtypes = [P, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
        lib.mf_plan_set_heldout.argtypes = [P, C.c_int64, P, P, P]
        lib.mf_plan_loss.argtypes = [P, C.c_int, C.POINTER(Loss), P]
        lib.mf_backend_loss_total.argtypes = [P, C.c_int32, C.c_int32, C.POINTER(C.c_double)]
        lib.mf_plan_iterate_monitored.argtypes = [P, C.c_int, C.c_int, C.c_double, C.POINTER(LossPoint), C.c_int,
                                                  C.POINTER(C.c_int), C.POINTER(C.c_int)]
        lib.mf_backend_loss.argtypes = [C.POINTER(Problem), P, P, C.POINTER(Loss), P, C.c_int]
        lib.mf_plan_rank_heldout.argtypes = [P, P]
        lib.mf_plan_rank_heldout_info.argtypes = [P, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
        lib.mf_backend_rank_metrics.argtypes = [P, P, C.c_int64, C.c_int32, C.POINTER(RankMetrics)]
        lib.mf_plan_similar_items.argtypes = [P, C.c_int, P, C.c_int32, C.c_int32, P, P]
        lib.mf_plan_similar_items_info.argtypes = [P, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
        lib.mf_backend_similar_items.argtypes = [P, C.c_int32, C.c_int32, C.c_int, P, C.c_int32, C.c_int32, P, P, C.c_int]
        lib.mf_plan_set_regularization.argtypes = [P, C.c_double, C.c_double]
        lib.mf_plan_get_regularization.argtypes = [P, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        lib.mf_plan_penalty.argtypes = [P, C.POINTER(C.c_double), C.POINTER(C.c_double), P, P]
        lib.mf_backend_run_reg.argtypes = [C.POINTER(Problem), _f64p, _f64p, P, C.c_double, C.c_double, C.c_int]
        lib.mf_plan_set_frozen_columns.argtypes = [P, C.c_int32, C.c_int32]
        lib.mf_plan_get_frozen_columns.argtypes = [P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        lib.mf_backend_bias_mean.argtypes = [P, C.c_int64, C.POINTER(C.c_double)]
        lib.mf_backend_bias_pack.argtypes = [P, P, C.c_int32, C.c_int32, C.c_int, P]
        lib.mf_backend_bias_unpack.argtypes = [P, C.c_int32, C.c_int32, C.c_int, P, P]
        lib.mf_backend_run_biased.argtypes = [C.POINTER(Problem), _f64p, _f64p, _f64p, _f64p, C.POINTER(C.c_double), P,
                                              C.c_double, C.c_double, C.c_int]
        lib.mf_plan_set_momentum.argtypes = [P, C.c_double, C.c_double]
        lib.mf_plan_get_momentum.argtypes = [P, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        lib.mf_plan_upload_previous.argtypes = [P, P, P]
        lib.mf_plan_download_previous.argtypes = [P, P, P]
        lib.mf_backend_run_momentum.argtypes = [C.POINTER(Problem), _f64p, _f64p, P, C.c_double, C.c_double, C.c_double, C.c_double,
                                                C.c_int]
        lib.mf_plan_create_weighted.argtypes = [C.POINTER(P), C.POINTER(Shard), P]
        lib.mf_plan_weight_total.argtypes = [P, C.POINTER(C.c_double), P]
        lib.mf_backend_run_weighted.argtypes = [C.POINTER(Problem), P, P, P, P, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int]
        lib.mf_plan_set_bounds.argtypes = [P, C.c_int, C.c_double, C.c_double, C.c_int32]
        lib.mf_plan_get_bounds.argtypes = [P, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32)]
        lib.mf_plan_project.argtypes = [P, C.c_int, C.c_int]
        lib.mf_plan_bounds_active.argtypes = [P, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        lib.mf_backend_run_bounded.argtypes = [C.POINTER(Problem), P, P, P, P, C.c_double, C.c_double, C.c_double, C.c_double,
                                               C.POINTER(Bounds), C.POINTER(Bounds), C.c_int]
        lib.mf_plan_set_adaptive.argtypes = [P, C.c_int, C.POINTER(Adaptive)]
        lib.mf_plan_get_adaptive.argtypes = [P, C.c_int, C.POINTER(Adaptive)]
        lib.mf_plan_reset_adaptive.argtypes = [P, C.c_int]
        lib.mf_plan_adaptive_finish.argtypes = [P, C.c_int]
        lib.mf_plan_download_adaptive_state.argtypes = [P, C.c_int, P, P, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double)]
        lib.mf_plan_upload_adaptive_state.argtypes = [P, C.c_int, P, P, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double)]
        lib.mf_backend_run_adaptive.argtypes = [C.POINTER(Problem), P, P, P, P, C.c_double, C.c_double, C.POINTER(Bounds), C.POINTER(Bounds),
                                                C.POINTER(Adaptive), C.POINTER(Adaptive), C.c_int]
        lib.mf_plan_set_als.argtypes = [P, C.c_int]
        lib.mf_plan_get_als.argtypes = [P, C.POINTER(C.c_int)]
        lib.mf_plan_als_solve.argtypes = [P, C.c_int, C.c_int]
        lib.mf_plan_als_info.argtypes = [P, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        lib.mf_backend_run_als.argtypes = [C.POINTER(Problem), P, P, P, P, C.c_double, C.c_double, C.POINTER(Bounds), C.POINTER(Bounds),
                                           C.c_int, C.c_int]
        lib.mf_plan_gram.argtypes = [P, C.c_int, C.c_int, P]
        lib.mf_plan_set_confidence.argtypes = [P, C.c_double]
        lib.mf_plan_get_confidence.argtypes = [P, C.POINTER(C.c_double)]
        lib.mf_plan_implicit_objective.argtypes = [P, C.POINTER(ImplicitObjective)]
        lib.mf_backend_gram_dot.argtypes = [P, P, C.c_int32, C.POINTER(C.c_double)]
        lib.mf_backend_run_implicit.argtypes = [C.POINTER(Problem), P, P, P, P, C.c_double, C.c_double, C.POINTER(Bounds),
                                                C.POINTER(Bounds), C.c_double, C.c_int]
        lib.mf_plan_set_als_cg.argtypes = [P, C.c_int]
        lib.mf_plan_get_als_cg.argtypes = [P, C.POINTER(C.c_int)]
        lib.mf_backend_run_als_cg.argtypes = [C.POINTER(Problem), P, P, P, P, C.c_double, C.c_double, C.POINTER(Bounds), C.POINTER(Bounds),
                                              C.c_int, C.c_int, C.c_int]
        lib.mf_backend_als_normal_pitch.argtypes = [C.c_int32]
        lib.mf_backend_als_normal_pitch.restype = C.c_int64
        lib.mf_plan_als_normal.argtypes = [P, C.c_int, C.c_int, P, C.c_int64]
        lib.mf_plan_als_solve_normal.argtypes = [P, C.c_int, P, C.c_int64]
        lib.mf_plan_set_implicit_cg.argtypes = [P, C.c_int]
        lib.mf_plan_get_implicit_cg.argtypes = [P, C.POINTER(C.c_int)]
        lib.mf_backend_run_implicit_cg.argtypes = [C.POINTER(Problem), P, P, P, P, C.c_double, C.c_double, C.POINTER(Bounds),
                                                   C.POINTER(Bounds), C.c_double, C.c_int, C.c_int]
        lib.mf_plan_set_als_box.argtypes = [P, C.c_int]
        lib.mf_plan_get_als_box.argtypes = [P, C.POINTER(C.c_int)]
        lib.mf_backend_run_als_box.argtypes = [C.POINTER(Problem), P, P, P, P, C.c_double, C.c_double, C.POINTER(Bounds), C.POINTER(Bounds),
                                               C.c_int, C.c_double, C.c_int, C.c_int]
        _hip = lib
    return _hip


def host():
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB_PATH):
            raise ImportError("%s is missing: run __graft_entry__.build()" % HOST_LIB_PATH)
        lib = C.CDLL(HOST_LIB_PATH)
        lib.mf_host_parse_strerror.restype = C.c_char_p
        lib.mf_host_parse_strerror.argtypes = [C.c_int]
        lib.mf_host_parse_file.argtypes = [C.c_char_p, C.POINTER(Problem)]
        lib.mf_host_parse_file_cached.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(Problem), C.POINTER(C.c_int)]
        lib.mf_host_parse_buffer.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(Problem)]
        lib.mf_host_free_problem.argtypes = [C.POINTER(Problem)]
        lib.mf_host_free_problem.restype = None
        lib.mf_host_srandom.argtypes = [C.POINTER(Rand), C.c_uint]
        lib.mf_host_srandom.restype = None
        lib.mf_host_random.argtypes = [C.POINTER(Rand)]
        lib.mf_host_random.restype = C.c_int32
        lib.mf_host_init_factors.argtypes = [C.c_int, C.c_int, C.c_int, _f64p, _f64p]
        lib.mf_host_init_factors.restype = None
        lib.mf_host_init_factors_block.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _f64p, C.c_void_p]
        lib.mf_host_init_factors_block.restype = None
        lib.mf_host_split_entries.argtypes = [C.POINTER(Entry), C.c_int64, _i32p, _i32p, _f64p]
        lib.mf_host_split_entries.restype = None
        lib.mf_host_partition_users.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, _i32p]
        lib.mf_host_balanced_grid.argtypes = [C.c_int, C.c_int, C.c_int, _i32p]
        lib.mf_host_synth_counts.argtypes = [C.POINTER(Synth), C.c_int, C.c_int, _i32p]
        lib.mf_host_synth_counts.restype = C.c_int64
        lib.mf_host_synth_fill.argtypes = [C.POINTER(Synth), C.c_int, C.c_int, _i32p, _i32p, _i32p, _f64p]
        lib.mf_host_write_topn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        _host = lib
    return _host


def _check(status, where):
    if status != MF_OK:
        raise HipBackendError(status, where)


# ------------------------------------------------------------------------------------ host helpers
class Instance:
    """A parsed instance in SoA form (what mf_shard wants)."""

    def __init__(self, iters, alpha, feats, users, items, row, col, val):
        self.iters, self.alpha, self.feats = int(iters), float(alpha), int(feats)
        self.users, self.items = int(users), int(items)
        self.row = np.ascontiguousarray(row, np.int32)
        self.col = np.ascontiguousarray(col, np.int32)
        self.val = np.ascontiguousarray(val, np.float64)

    @property
    def nnz(self):
        return int(self.row.shape[0])


class ParseError(ValueError):
    def __init__(self, status):
        self.status = status
        super().__init__(host().mf_host_parse_strerror(status).decode())


def parse_file(path):
    """`.in` reader through the C parser (mf_host_parse_file); gz files are inflated first."""
    if str(path).endswith(".gz"):
        import gzip
        with gzip.open(path, "rb") as f:
            return parse_text(f.read())
    p = Problem()
    rc = host().mf_host_parse_file(os.fsencode(path), C.byref(p))
    if rc != 0:
        raise ParseError(rc)
    return _from_problem(p)


def parse_file_cached(path, cache_dir):
    """(instance, cache_hit) through the binary cache of mf_host_parse_file_cached."""
    p = Problem()
    hit = C.c_int(0)
    rc = host().mf_host_parse_file_cached(os.fsencode(path), os.fsencode(cache_dir), C.byref(p), C.byref(hit))
    if rc != 0:
        raise ParseError(rc)
    return _from_problem(p), bool(hit.value)


def parse_text(text):
    if isinstance(text, str):
        text = text.encode()
    p = Problem()
    rc = host().mf_host_parse_buffer(text, len(text), C.byref(p))
    if rc != 0:
        raise ParseError(rc)
    return _from_problem(p)


def _from_problem(p):
    n = int(p.nnz)
    row, col, val = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.float64)
    host().mf_host_split_entries(p.entries, n, row, col, val)
    inst = Instance(p.iters, p.alpha, p.features, p.users, p.items, row, col, val)
    host().mf_host_free_problem(C.byref(p))
    return inst


def init_factors(users, items, feats):
    """Initial L (users x K) and R (items x K): mat2d_random_fill_LR + transpose, own glibc random()."""
    L = np.empty((users, feats), np.float64)
    R = np.empty((items, feats), np.float64)
    host().mf_host_init_factors(users, items, feats, L, R)
    return L, R


def init_factors_block(users, items, feats, u0, count, want_r=True):
    Lb = np.empty((count, feats), np.float64)
    R = np.empty((items, feats), np.float64) if want_r else None
    host().mf_host_init_factors_block(users, items, feats, u0, count, Lb,
                                      R.ctypes.data if R is not None else None)
    return Lb, R


def partition_users(users, parts, row_ptr=None):
    """begin[0..parts]; by entry count when the CSR row pointer (int64, users+1) is given, else BLOCK_LOW."""
    begin = np.empty(parts + 1, np.int32)
    if row_ptr is not None:
        row_ptr = np.ascontiguousarray(row_ptr, np.int64)
        rc = host().mf_host_partition_users(users, parts, 1, row_ptr.ctypes.data, begin)
    else:
        rc = host().mf_host_partition_users(users, parts, 0, None, begin)
    if rc != 0:
        raise ValueError("mf_host_partition_users failed")
    return begin


def row_pitch(feats):
    """Row pitch (doubles) the backend gives factor buffers it owns for this K (K, or K padded to whole 128-byte
    lines); caller-owned buffers may use the same and declare it (Plan(items_pitch=..., users_pitch=...))."""
    return int(hip().mf_backend_row_pitch(int(feats)))


def recommend_margin(feats):
    """8*(K+8)*2^-53: the factor of ||l||*||r|| above which a matrix-core score gap certifies the arg-max."""
    return float(hip().mf_backend_recommend_margin(int(feats)))


def balanced_grid(users, items, nproc):
    """(grid rows, grid cols) of the reference's 2-D process grid (create_balanced_grid, mpiutil.c:54-88)."""
    size = np.empty(2, np.int32)
    if host().mf_host_balanced_grid(int(users), int(items), int(nproc), size) != 0:
        raise ValueError("mf_host_balanced_grid failed")
    return int(size[0]), int(size[1])


def synth_counts(seed, users, items, min_row, max_row, u0=0, count=None, columns="stratified", target_nnz=0):
    count = users - u0 if count is None else count
    s = Synth(seed, users, items, min_row, max_row, SYNTH_MODES[columns], 0, int(target_nnz))
    counts = np.empty(count, np.int32)
    total = host().mf_host_synth_counts(C.byref(s), u0, count, counts)
    return counts, int(total)


def synth_block(seed, users, items, min_row, max_row, u0=0, count=None, columns="stratified", target_nnz=0):
    """(row, col, val) of users [u0, u0+count) of the synthetic instance, (row, col)-sorted.  columns: "stratified" (one
    column per stratum), "uniform" (distinct uniform columns) or "zipf" (Zipf(1.0) item popularity); target_nnz > 0
    rescales the row counts so that the WHOLE instance has exactly that many entries."""
    count = users - u0 if count is None else count
    counts, total = synth_counts(seed, users, items, min_row, max_row, u0, count, columns, target_nnz)
    row, col, val = np.empty(total, np.int32), np.empty(total, np.int32), np.empty(total, np.float64)
    s = Synth(seed, users, items, min_row, max_row, SYNTH_MODES[columns], 0, int(target_nnz))
    if host().mf_host_synth_fill(C.byref(s), u0, count, counts, row, col, val) != 0:
        raise MemoryError("mf_host_synth_fill")
    return row, col, val


def device_count():
    return hip().mf_backend_device_count()


def file_sha256(path):
    import hashlib
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 20), b""):
            h.update(blk)
    return h.hexdigest()


def kernel_source_hash():
    """Hash (16 hex digits) of the kernel sources under csrc/: measurements kept in files (PMC traffic) are tied to
    it, so a record is never quoted for kernels it was not measured on."""
    import glob
    import hashlib
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(_HERE, "csrc", "*.hip")) + glob.glob(os.path.join(_HERE, "csrc", "*.hip.h"))):
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


# ------------------------------------------------------------------------------------ level 1
def _problem(inst, iters=None):
    ent = (Entry * max(inst.nnz, 1))()
    buf = np.ctypeslib.as_array(ent).view(np.dtype([("row", np.int32), ("col", np.int32), ("value", np.float64)]))
    buf["row"][:inst.nnz] = inst.row
    buf["col"][:inst.nnz] = inst.col
    buf["value"][:inst.nnz] = inst.val
    p = Problem(inst.users, inst.items, inst.feats, inst.iters if iters is None else iters, inst.alpha,
                inst.nnz, ent)
    return p, ent


def backend_run(inst, L, R, iters=None, device=0):
    """mf_backend_run: L, R updated in place, returns best[users]."""
    p, keep = _problem(inst, iters)
    best = np.empty(inst.users, np.int32)
    _check(hip().mf_backend_run(C.byref(p), L, R, best, device), "mf_backend_run")
    return best


def backend_run_reg(inst, L, R, lambda_users, lambda_items=None, iters=None, device=0, recommend=True):
    """mf_backend_run_reg: backend_run under L2 regularisation (one value means both sides); L, R updated in place,
    returns best[users], or None with recommend=False."""
    p, keep = _problem(inst, iters)
    li = lambda_users if lambda_items is None else lambda_items
    best = np.empty(inst.users, np.int32) if recommend else None
    _check(hip().mf_backend_run_reg(C.byref(p), L, R, best.ctypes.data if recommend else None, float(lambda_users), float(li),
                                    device), "mf_backend_run_reg")
    return best


def backend_run_momentum(inst, L, R, lambda_users, lambda_items, beta_users, beta_items=None, iters=None, device=0, recommend=True):
    """mf_backend_run_momentum: backend_run_reg with heavy-ball momentum from rest (one beta means both sides); L, R updated
    in place, returns best[users], or None with recommend=False."""
    p, keep = _problem(inst, iters)
    bi = beta_users if beta_items is None else beta_items
    best = np.empty(inst.users, np.int32) if recommend else None
    _check(hip().mf_backend_run_momentum(C.byref(p), L, R, best.ctypes.data if recommend else None, float(lambda_users),
                                         float(lambda_items), float(beta_users), float(bi), device), "mf_backend_run_momentum")
    return best


run_momentum = backend_run_momentum


def backend_run_weighted(inst, weight, L, R, lambda_users=0.0, lambda_items=None, beta_users=0.0, beta_items=None, iters=None, device=0,
                         recommend=True):
    """mf_backend_run_weighted: backend_run_momentum on a plan with one confidence weight per entry (weight: inst.nnz doubles
    in the entries' order, or None for an unweighted run); L, R updated in place, returns best[users], or None with
    recommend=False."""
    p, keep = _problem(inst, iters)
    w = None if weight is None else np.ascontiguousarray(weight, np.float64)
    assert w is None or w.shape == (inst.nnz,)
    li = lambda_users if lambda_items is None else lambda_items
    bi = beta_users if beta_items is None else beta_items
    best = np.empty(inst.users, np.int32) if recommend else None
    assert L.dtype == np.float64 and R.dtype == np.float64 and L.flags.c_contiguous and R.flags.c_contiguous
    _check(hip().mf_backend_run_weighted(C.byref(p), None if w is None else w.ctypes.data, L.ctypes.data, R.ctypes.data,
                                         best.ctypes.data if recommend else None,
                                         float(lambda_users), float(li), float(beta_users), float(bi), device), "mf_backend_run_weighted")
    return best


run_weighted = backend_run_weighted

SIDES = {"items": 0, "users": 1, 0: 0, 1: 1}
GENERATIONS = {"current": 0, "next": 1, 0: 0, 1: 1}


def _bounds_record(b):
    """mf_bounds from None (unbounded), (lo, hi) or (lo, hi, columns)"""
    if b is None:
        return None
    lo, hi = float(b[0]), float(b[1])
    return Bounds(lo, hi, int(b[2]) if len(b) > 2 else -1)


def _run_boxed(name, inst, L, R, weight, lambda_users, lambda_items, bounds_users, bounds_items, iters, device, recommend, *tail,
               betas=()):
    """What the level-1 runs with a box per side share: mf_backend_run_<name>(problem, weight, L, R, best, the lambdas (one
    value means both sides), `betas`, the bounds records, `tail`, device), checked; returns best[users] or None."""
    p, keep = _problem(inst, iters)
    w = None if weight is None else np.ascontiguousarray(weight, np.float64)
    assert w is None or w.shape == (inst.nnz,)
    li = lambda_users if lambda_items is None else lambda_items
    bu, bit = _bounds_record(bounds_users), _bounds_record(bounds_items)
    best = np.empty(inst.users, np.int32) if recommend else None
    assert L.dtype == np.float64 and R.dtype == np.float64 and L.flags.c_contiguous and R.flags.c_contiguous
    fn = "mf_backend_run_" + name
    _check(getattr(hip(), fn)(C.byref(p), None if w is None else w.ctypes.data, L.ctypes.data, R.ctypes.data,
                              best.ctypes.data if recommend else None, float(lambda_users), float(li), *betas,
                              None if bu is None else C.byref(bu), None if bit is None else C.byref(bit), *tail, device), fn)
    return best


def backend_run_bounded(inst, L, R, bounds_users=None, bounds_items=None, weight=None, lambda_users=0.0, lambda_items=None,
                        beta_users=0.0, beta_items=None, iters=None, device=0, recommend=True):
    """mf_backend_run_bounded: backend_run_weighted with a box per side -- None (unbounded), (lo, hi) over all columns or
    (lo, hi, columns) over the leading `columns`; a finished row is projected onto it in every seeded sweep.  L, R updated in
    place, returns best[users], or None with recommend=False."""
    bi = beta_users if beta_items is None else beta_items
    return _run_boxed("bounded", inst, L, R, weight, lambda_users, lambda_items, bounds_users, bounds_items, iters, device, recommend,
                      betas=(float(beta_users), float(bi)))


run_bounded = backend_run_bounded


def _adaptive_record(a):
    """mf_adaptive from None (the plain step), an Adaptive, or (kind, eta[, beta1, beta2[, eps]]) with the defaults of
    Plan.set_adaptive"""
    if a is None or isinstance(a, Adaptive):
        return a
    kind, eta = a[0], a[1]
    b1, b2 = (a[2], a[3]) if len(a) > 3 else (0.9, 0.999)
    return Adaptive(OPTIMIZERS[kind], float(eta), float(b1), float(b2), float(a[4]) if len(a) > 4 else 1e-8)


def backend_run_adaptive(inst, L, R, adaptive_users=None, adaptive_items=None, bounds_users=None, bounds_items=None, weight=None,
                         lambda_users=0.0, lambda_items=None, iters=None, device=0, recommend=True):
    """mf_backend_run_adaptive: backend_run_bounded without momentum and with an adaptive rule per side -- None (the plain
    step) or (kind, eta[, beta1, beta2[, eps]]), kind "adam" | "rmsprop" | "adagrad".  L, R updated in place, returns
    best[users], or None with recommend=False."""
    au, ai = _adaptive_record(adaptive_users), _adaptive_record(adaptive_items)
    return _run_boxed("adaptive", inst, L, R, weight, lambda_users, lambda_items, bounds_users, bounds_items, iters, device, recommend,
                      None if au is None else C.byref(au), None if ai is None else C.byref(ai))


run_adaptive = backend_run_adaptive


def backend_run_als(inst, L, R, kind="ridge", bounds_users=None, bounds_items=None, weight=None, lambda_users=0.0, lambda_items=None,
                    iters=None, device=0, recommend=True):
    """mf_backend_run_als: `iters` ALS iterations (kind "ridge" | "ridge-count") from the factors in L and R, with a lambda and
    a box per side and optional per-entry weights.  L, R updated in place, returns best[users], or None with
    recommend=False."""
    return _run_boxed("als", inst, L, R, weight, lambda_users, lambda_items, bounds_users, bounds_items, iters, device, recommend,
                      ALS_KINDS.get(kind, kind))


run_als = backend_run_als


def backend_run_als_cg(inst, L, R, steps, kind="ridge", bounds_users=None, bounds_items=None, weight=None, lambda_users=0.0,
                       lambda_items=None, iters=None, device=0, recommend=True):
    """mf_backend_run_als_cg: backend_run_als with `steps` conjugate-gradient steps per row in place of the direct solve (0: the
    direct solve); K up to 256."""
    return _run_boxed("als_cg", inst, L, R, weight, lambda_users, lambda_items, bounds_users, bounds_items, iters, device, recommend,
                      ALS_KINDS.get(kind, kind), int(steps))


run_als_cg = backend_run_als_cg


def backend_run_implicit(inst, L, R, conf=1.0, bounds_users=None, bounds_items=None, weight=None, lambda_users=0.0, lambda_items=None,
                         iters=None, device=0, recommend=True):
    """mf_backend_run_implicit: `iters` implicit-feedback ALS iterations at confidence 1 + conf * w from the factors in L and R,
    with a lambda and a box per side and optional per-entry weights.  L, R updated in place, returns best[users], or None
    with recommend=False."""
    return _run_boxed("implicit", inst, L, R, weight, lambda_users, lambda_items, bounds_users, bounds_items, iters, device, recommend,
                      float(conf))


run_implicit = backend_run_implicit


def backend_run_implicit_cg(inst, L, R, steps, conf=1.0, bounds_users=None, bounds_items=None, weight=None, lambda_users=0.0,
                            lambda_items=None, iters=None, device=0, recommend=True):
    """mf_backend_run_implicit_cg: backend_run_implicit with `steps` conjugate-gradient steps per row in place of the direct
    solve (0: the direct solve)."""
    return _run_boxed("implicit_cg", inst, L, R, weight, lambda_users, lambda_items, bounds_users, bounds_items, iters, device, recommend,
                      float(conf), int(steps))


run_implicit_cg = backend_run_implicit_cg


def backend_run_als_box(inst, L, R, sweeps, kind="ridge", conf=1.0, bounds_users=None, bounds_items=None, weight=None, lambda_users=0.0,
                        lambda_items=None, iters=None, device=0, recommend=True):
    """mf_backend_run_als_box: `iters` ALS iterations of `kind` ("ridge" | "ridge-count" | "implicit", conf read under the last)
    with `sweeps` coordinate-descent sweeps per row in place of Cholesky and the clamp (0: the direct solve)."""
    return _run_boxed("als_box", inst, L, R, weight, lambda_users, lambda_items, bounds_users, bounds_items, iters, device, recommend,
                      ALS_KINDS.get(kind, kind), float(conf), int(sweeps))


run_als_box = backend_run_als_box


def als_normal_pitch(feats):
    """mf_backend_als_normal_pitch: doubles of one normal record, the smallest even number >= K (K + 1) / 2 + K + 1"""
    return int(hip().mf_backend_als_normal_pitch(int(feats)))


def gram_dot(left, right):
    """mf_backend_gram_dot: the sum of the elementwise products of two symmetric K x K matrices given as packed lower triangles,
    over the full matrices, p ascending then q ascending, from 0.0"""
    left, right = np.ascontiguousarray(left, np.float64), np.ascontiguousarray(right, np.float64)
    K = int((np.sqrt(8 * left.size + 1) - 1) // 2)
    assert left.shape == right.shape == (K * (K + 1) // 2,)
    out = C.c_double()
    _check(hip().mf_backend_gram_dot(left.ctypes.data, right.ctypes.data, K, C.byref(out)), "mf_backend_gram_dot")
    return out.value


def bias_mean(val):
    """mf_backend_bias_mean: the mean of `val` summed in the given order from 0.0; 0.0 for an empty array."""
    v = np.ascontiguousarray(val, np.float64)
    mu = C.c_double()
    _check(hip().mf_backend_bias_mean(v.ctypes.data, v.size, C.byref(mu)), "mf_backend_bias_mean")
    return mu.value


def bias_pack(X, bias, side):
    """mf_backend_bias_pack: rows x (F+2) -- side 1 (users) [X | bias | 1.0], side 0 (items) [X | 1.0 | bias]; bias=None
    means zeros."""
    X = np.ascontiguousarray(X, np.float64)
    rows, F = X.shape
    b = None if bias is None else np.ascontiguousarray(bias, np.float64)
    if b is not None and b.shape != (rows,):
        raise ValueError("bias_pack: bias must have one element per row")
    out = np.empty((rows, F + 2), np.float64)
    _check(hip().mf_backend_bias_pack(X.ctypes.data, None if b is None else b.ctypes.data, rows, F, int(side), out.ctypes.data),
           "mf_backend_bias_pack")
    return out


def bias_unpack(packed, side):
    """mf_backend_bias_unpack: (X, bias) of a packed rows x (F+2) factor."""
    p = np.ascontiguousarray(packed, np.float64)
    rows, K = p.shape
    X, b = np.empty((rows, K - 2), np.float64), np.empty(rows, np.float64)
    _check(hip().mf_backend_bias_unpack(p.ctypes.data, rows, K - 2, int(side), X.ctypes.data, b.ctypes.data),
           "mf_backend_bias_unpack")
    return X, b


def backend_run_biased(inst, L, R, user_bias, item_bias, lambda_users=0.0, lambda_items=None, iters=None, device=0,
                       recommend=True):
    """mf_backend_run_biased: the model a ~ mu + b_user + b_item + l.r; L, R (inst.feats latent columns), user_bias and
    item_bias are updated in place.  Returns (mu, best), best None with recommend=False."""
    p, keep = _problem(inst, iters)
    li = lambda_users if lambda_items is None else lambda_items
    best = np.empty(inst.users, np.int32) if recommend else None
    mu = C.c_double()
    _check(hip().mf_backend_run_biased(C.byref(p), L, R, user_bias, item_bias, C.byref(mu),
                                       best.ctypes.data if recommend else None, float(lambda_users), float(li), device),
           "mf_backend_run_biased")
    return mu.value, best


def backend_run_multi(inst, L, R, devices, iters=None):
    """mf_backend_run_multi: one process, len(devices) shards (ordinals may repeat)."""
    p, keep = _problem(inst, iters)
    best = np.empty(inst.users, np.int32)
    dev = np.ascontiguousarray(devices, np.int32)
    _check(hip().mf_backend_run_multi(C.byref(p), L, R, best, dev, len(dev)), "mf_backend_run_multi")
    return best


def multi_last_timing():
    """Host wall-clock and counters of the last backend_run_multi: dict(setup_s, iterate_s, recommend_s, shards, reducer,
    sliced, enqueue_s, entry_passes, host_threads)."""
    a, b, c, e = C.c_double(), C.c_double(), C.c_double(), C.c_double()
    info = (C.c_int * 3)()
    passes, threads = C.c_int64(), C.c_int()
    _check(hip().mf_backend_multi_last_timing(C.byref(a), C.byref(b), C.byref(c), C.byref(info)),
           "mf_backend_multi_last_timing")
    _check(hip().mf_backend_multi_last_counters(C.byref(e), C.byref(passes), C.byref(threads)),
           "mf_backend_multi_last_counters")
    return {"setup_s": a.value, "iterate_s": b.value, "recommend_s": c.value, "shards": info[0],
            "reducer": "rccl" if info[1] else "peer", "sliced": bool(info[2]), "enqueue_s": e.value,
            "entry_passes": passes.value, "host_threads": threads.value}


def backend_run_top1(inst, L0, R0, iters=None, device=0):
    """mf_backend_run_top1: initial factors in, only the recommendation list out."""
    p, keep = _problem(inst, iters)
    best = np.empty(inst.users, np.int32)
    _check(hip().mf_backend_run_top1(C.byref(p), L0, R0, best, device), "mf_backend_run_top1")
    return best


def backend_factorize(inst, L, R, iters=None, device=0):
    p, keep = _problem(inst, iters)
    _check(hip().mf_backend_factorize(C.byref(p), L, R, device), "mf_backend_factorize")


def backend_recommend(inst, L, R, device=0):
    p, keep = _problem(inst)
    best = np.empty(inst.users, np.int32)
    _check(hip().mf_backend_recommend(C.byref(p), L, R, best, device), "mf_backend_recommend")
    return best


def _topn(entry, inst, L, R, n, iters=None, device=0):
    p, keep = _problem(inst, iters)
    L = np.ascontiguousarray(L, np.float64)
    R = np.ascontiguousarray(R, np.float64)
    items = np.empty((inst.users, max(int(n), 0)), np.int32)
    scores = np.empty((inst.users, max(int(n), 0)), np.float64)
    _check(getattr(hip(), entry)(C.byref(p), L.ctypes.data, R.ctypes.data, int(n), items.ctypes.data, scores.ctypes.data,
                                 device), entry)
    return items, scores


def backend_recommend_topn(inst, L, R, n, device=0):
    """mf_backend_recommend_topn: (items, scores), users x n; item -1 / score NaN past the user's unrated items."""
    return _topn("mf_backend_recommend_topn", inst, L, R, n, device=device)


def backend_run_topn(inst, L0, R0, n, iters=None, device=0):
    """mf_backend_run_topn: initial factors in, (items, scores) of the top-N lists out (no copy-back of the factors)."""
    return _topn("mf_backend_run_topn", inst, L0, R0, n, iters=iters, device=device)


def write_topn(items):
    """mf_host_write_topn of an (users x n) int32 array, as bytes."""
    import tempfile
    items = np.ascontiguousarray(items, np.int32)
    libc = C.CDLL(None)
    libc.fdopen.restype = C.c_void_p
    libc.fdopen.argtypes = [C.c_int, C.c_char_p]
    libc.fclose.argtypes = [C.c_void_p]
    with tempfile.TemporaryFile() as tf:
        f = libc.fdopen(os.dup(tf.fileno()), b"w")
        rc = host().mf_host_write_topn(f, items.ctypes.data, items.shape[0], items.shape[1])
        libc.fclose(f)
        if rc != 0:
            raise ValueError("mf_host_write_topn failed")
        tf.seek(0)
        return tf.read()


def backend_loss(inst, L, R, rows=False, device=0):
    """mf_backend_loss: the training loss of these factors as a Loss (sse, count, rmse); with rows=True also the row sums."""
    p, keep = _problem(inst, None)
    L = np.ascontiguousarray(L, np.float64)
    R = np.ascontiguousarray(R, np.float64)
    out = Loss()
    rs = np.empty(inst.users, np.float64) if rows else None
    _check(hip().mf_backend_loss(C.byref(p), L.ctypes.data, R.ctypes.data, C.byref(out), rs.ctypes.data if rows else None,
                                 device), "mf_backend_loss")
    return (out, rs) if rows else out


def loss_total(row_sse, user_begin=0):
    """mf_backend_loss_total: step 4 of the loss contract over the row sums of consecutive users from user_begin (host only)."""
    row_sse = np.ascontiguousarray(row_sse, np.float64)
    sse = C.c_double()
    _check(hip().mf_backend_loss_total(row_sse.ctypes.data, int(user_begin), int(row_sse.shape[0]), C.byref(sse)),
           "mf_backend_loss_total")
    return sse.value


def rank_metrics(rank, row, cutoff):
    """mf_backend_rank_metrics: hit rate, MRR and NDCG at `cutoff` of a rank vector (Plan.rank_heldout) and the users of its
    entries, as a RankMetrics (host only)."""
    rank = np.ascontiguousarray(rank, np.int32)
    row = np.ascontiguousarray(row, np.int32)
    assert rank.shape == row.shape and rank.ndim == 1
    out = RankMetrics()
    _check(hip().mf_backend_rank_metrics(rank.ctypes.data, row.ctypes.data, int(rank.shape[0]), int(cutoff), C.byref(out)),
           "mf_backend_rank_metrics")
    return out


def _similar_query(query, items):
    """(contiguous int32 query or None, its pointer, nq) of a similar-items call"""
    if query is None:
        return None, None, int(items)
    query = np.ascontiguousarray(query, np.int32)
    assert query.ndim == 1
    return query, query.ctypes.data, int(query.shape[0])


def backend_similar_items(R, n, metric="cosine", query=None, device=0):
    """mf_backend_similar_items: (items, scores), one row of n per query item (all items in ascending order with
    query=None); item -1 / score NaN past the other items.  metric: "cosine", "dot" or one of the MF_SIMILAR_* codes."""
    R = np.ascontiguousarray(R, np.float64)
    assert R.ndim == 2
    query, qptr, nq = _similar_query(query, R.shape[0])
    items = np.empty((nq, max(int(n), 0)), np.int32)
    scores = np.empty((nq, max(int(n), 0)), np.float64)
    _check(hip().mf_backend_similar_items(R.ctypes.data, R.shape[0], R.shape[1], int(SIMILAR_METRICS.get(metric, metric)), qptr,
                                          nq, int(n), items.ctypes.data, scores.ctypes.data, device),
           "mf_backend_similar_items")
    return items, scores


# ------------------------------------------------------------------------------------ level 2
class Plan:
    """mf_plan: one shard resident on one GPU.  weight: one confidence weight per entry, in the order of row / col / val
    (mf_plan_create_weighted); None: an unweighted plan (mf_plan_create)."""

    def __init__(self, users_total, items, feats, alpha, row, col, val, user_begin=0, user_count=None,
                 device=0, items_ext=None, flags=0, users_ext=None, items_pitch=0, users_pitch=0, weight=None):
        self.users_total, self.items, self.feats = int(users_total), int(items), int(feats)
        self.user_begin = int(user_begin)
        self.user_count = int(users_total - user_begin if user_count is None else user_count)
        self._keep = (np.ascontiguousarray(row, np.int32), np.ascontiguousarray(col, np.int32),
                      np.ascontiguousarray(val, np.float64))
        s = Shard()
        s.users_total, s.items, s.features = self.users_total, self.items, self.feats
        s.user_begin, s.user_count = self.user_begin, self.user_count
        s.nnz = int(self._keep[0].shape[0])
        s.row, s.col, s.val = (a.ctypes.data for a in self._keep)
        s.alpha, s.device, s.flags = float(alpha), int(device), int(flags)
        if items_ext is not None:
            s.items_ext[0], s.items_ext[1] = int(items_ext[0]), int(items_ext[1])
        if users_ext is not None:
            s.users_ext[0], s.users_ext[1] = int(users_ext[0]), int(users_ext[1])
        s.items_pitch, s.users_pitch = int(items_pitch), int(users_pitch)
        self.nnz = s.nnz
        self._h = C.c_void_p()
        if weight is None:
            _check(hip().mf_plan_create(C.byref(self._h), C.byref(s)), "mf_plan_create")
        else:
            w = np.ascontiguousarray(weight, np.float64)
            assert w.shape == (s.nnz,)
            _check(hip().mf_plan_create_weighted(C.byref(self._h), C.byref(s), w.ctypes.data), "mf_plan_create_weighted")
        self.weighted = weight is not None
        self._keep = None  # the plan copied everything it needs into HBM

    def close(self):
        if getattr(self, "_h", None):
            hip().mf_plan_destroy(self._h)
            self._h = None

    __del__ = close

    def set_stream(self, stream_ptr):
        _check(hip().mf_plan_set_stream(self._h, stream_ptr), "mf_plan_set_stream")

    def upload(self, L_block, R):
        L_block = np.ascontiguousarray(L_block, np.float64)
        R = np.ascontiguousarray(R, np.float64)
        assert L_block.shape == (self.user_count, self.feats) and R.shape == (self.items, self.feats)
        _check(hip().mf_plan_upload_factors(self._h, L_block.ctypes.data, R.ctypes.data), "mf_plan_upload_factors")

    def download(self, want_l=True, want_r=True):
        Lb = np.empty((self.user_count, self.feats), np.float64) if want_l else None
        R = np.empty((self.items, self.feats), np.float64) if want_r else None
        _check(hip().mf_plan_download_factors(self._h, Lb.ctypes.data if want_l else None,
                                              R.ctypes.data if want_r else None), "mf_plan_download_factors")
        return Lb, R

    def iterate(self, iters):
        _check(hip().mf_plan_iterate(self._h, int(iters)), "mf_plan_iterate")

    def weight_total(self, rows=False):
        """mf_plan_weight_total: the sum of the plan's weights -- per user in entry order, the rows then combined like the
        loss's row sums; (sum_w, row_w) with rows=True.  An unweighted plan raises MF_ERR_STATE."""
        total = C.c_double()
        rw = np.empty(self.user_count, np.float64) if rows else None
        _check(hip().mf_plan_weight_total(self._h, C.byref(total), rw.ctypes.data if rows else None), "mf_plan_weight_total")
        return (total.value, rw) if rows else total.value

    def set_regularization(self, users, items=None):
        """mf_plan_set_regularization: the L2 weights of the user and the item side (one value means both), in force from
        the next sweep or iterate call."""
        _check(hip().mf_plan_set_regularization(self._h, float(users), float(users if items is None else items)),
               "mf_plan_set_regularization")

    def regularization(self):
        """(lambda_users, lambda_items) in force"""
        u, i = C.c_double(), C.c_double()
        _check(hip().mf_plan_get_regularization(self._h, C.byref(u), C.byref(i)), "mf_plan_get_regularization")
        return u.value, i.value

    def set_momentum(self, users, items=None):
        """mf_plan_set_momentum: heavy-ball beta of the user and the item side (one value means both), read at every launch.
        A side whose beta leaves 0 is at rest: its first step sees X_prev = X_old."""
        _check(hip().mf_plan_set_momentum(self._h, float(users), float(users if items is None else items)), "mf_plan_set_momentum")

    def momentum(self):
        """(beta_users, beta_items) in force"""
        u, i = C.c_double(), C.c_double()
        _check(hip().mf_plan_get_momentum(self._h, C.byref(u), C.byref(i)), "mf_plan_get_momentum")
        return u.value, i.value

    def upload_previous(self, L_prev_block=None, R_prev=None):
        """mf_plan_upload_previous: the generation before the current one, into the next-generation buffers; None leaves
        that side alone.  A side given is no longer at rest."""
        Lp = None if L_prev_block is None else np.ascontiguousarray(L_prev_block, np.float64)
        Rp = None if R_prev is None else np.ascontiguousarray(R_prev, np.float64)
        assert Lp is None or Lp.shape == (self.user_count, self.feats)
        assert Rp is None or Rp.shape == (self.items, self.feats)
        _check(hip().mf_plan_upload_previous(self._h, None if Lp is None else Lp.ctypes.data, None if Rp is None else Rp.ctypes.data),
               "mf_plan_upload_previous")

    def download_previous(self, want_l=True, want_r=True):
        """mf_plan_download_previous: (L_prev_block, R_prev); a side at rest returns its current factors"""
        Lb = np.empty((self.user_count, self.feats), np.float64) if want_l else None
        R = np.empty((self.items, self.feats), np.float64) if want_r else None
        _check(hip().mf_plan_download_previous(self._h, Lb.ctypes.data if want_l else None, R.ctypes.data if want_r else None),
               "mf_plan_download_previous")
        return Lb, R

    def set_frozen_columns(self, users, items):
        """mf_plan_set_frozen_columns: the column of L and of R that the sweeps leave alone (-1: none), in force from the
        next sweep or iterate call."""
        _check(hip().mf_plan_set_frozen_columns(self._h, int(users), int(items)), "mf_plan_set_frozen_columns")

    def frozen_columns(self):
        """(users' column, items' column) in force; -1: none"""
        u, i = C.c_int32(), C.c_int32()
        _check(hip().mf_plan_get_frozen_columns(self._h, C.byref(u), C.byref(i)), "mf_plan_get_frozen_columns")
        return u.value, i.value

    def set_bounds(self, side, lo=-np.inf, hi=np.inf, columns=-1):
        """mf_plan_set_bounds: the box [lo, hi] over the leading `columns` columns (-1: all) of a side ("items" / 0 or
        "users" / 1), in force from the next launch; a seeded sweep projects every finished row onto it."""
        _check(hip().mf_plan_set_bounds(self._h, SIDES[side], float(lo), float(hi), int(columns)), "mf_plan_set_bounds")

    def bounds(self, side):
        """mf_plan_get_bounds: (lo, hi, columns) of a side"""
        lo, hi, n = C.c_double(), C.c_double(), C.c_int32()
        _check(hip().mf_plan_get_bounds(self._h, SIDES[side], C.byref(lo), C.byref(hi), C.byref(n)), "mf_plan_get_bounds")
        return lo.value, hi.value, n.value

    def project(self, side, generation="current"):
        """mf_plan_project: the side's current or next buffer projected onto its box in place (bounded, non-frozen columns)"""
        _check(hip().mf_plan_project(self._h, SIDES[side], GENERATIONS[generation]), "mf_plan_project")

    def bounds_active(self, side):
        """mf_plan_bounds_active: (at_lo, at_hi, inside) of the side's current factor over its bounded, non-frozen columns"""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        _check(hip().mf_plan_bounds_active(self._h, SIDES[side], C.byref(a), C.byref(b), C.byref(c)), "mf_plan_bounds_active")
        return a.value, b.value, c.value

    def set_adaptive(self, side, kind, eta=0.0, beta1=0.9, beta2=0.999, eps=1e-8):
        """mf_plan_set_adaptive: the adaptive rule of a side ("items" / 0 or "users" / 1) -- kind "adam", "rmsprop" (beta2 is
        its rho), "adagrad", or "none" / None for the plain step --, in force from the next launch.  A change of kind puts
        the side's accumulators at rest; a change of the numbers alone keeps them."""
        rec = Adaptive(OPTIMIZERS[kind], float(eta), float(beta1), float(beta2), float(eps))
        _check(hip().mf_plan_set_adaptive(self._h, SIDES[side], C.byref(rec)), "mf_plan_set_adaptive")

    def adaptive(self, side):
        """mf_plan_get_adaptive: (kind name, eta, beta1, beta2, eps) of a side; ("none", 0, 0, 0, 0) without a rule"""
        rec = Adaptive()
        _check(hip().mf_plan_get_adaptive(self._h, SIDES[side], C.byref(rec)), "mf_plan_get_adaptive")
        return OPTIMIZER_NAMES[rec.kind], rec.eta, rec.beta1, rec.beta2, rec.eps

    def reset_adaptive(self, side):
        """mf_plan_reset_adaptive: the side's accumulators back to rest (zeros, 1.0, 0 steps)"""
        _check(hip().mf_plan_reset_adaptive(self._h, SIDES[side]), "mf_plan_reset_adaptive")

    def adaptive_finish(self, side):
        """mf_plan_adaptive_finish: the side's next-generation buffer taken as g and finished in place: what a sharded caller
        runs on the summed side after its sum"""
        _check(hip().mf_plan_adaptive_finish(self._h, SIDES[side]), "mf_plan_adaptive_finish")

    def set_als(self, kind):
        """mf_plan_set_als: "ridge", "ridge-count", "implicit", or "off" / None for the gradient step; while it is on,
        iterate() runs ALS iterations (users against the current R, items against the new L, flip)"""
        _check(hip().mf_plan_set_als(self._h, ALS_KINDS.get(kind, kind)), "mf_plan_set_als")

    def als(self):
        """mf_plan_get_als: the kind by name"""
        k = C.c_int()
        _check(hip().mf_plan_get_als(self._h, C.byref(k)), "mf_plan_get_als")
        return ALS_KIND_NAMES[k.value]

    def set_als_cg(self, steps):
        """mf_plan_set_als_cg: conjugate-gradient steps per row of an ALS solve (0: the direct solve); read at every launch"""
        _check(hip().mf_plan_set_als_cg(self._h, int(steps)), "mf_plan_set_als_cg")

    def als_cg(self):
        """mf_plan_get_als_cg: the steps"""
        s = C.c_int()
        _check(hip().mf_plan_get_als_cg(self._h, C.byref(s)), "mf_plan_get_als_cg")
        return s.value

    def set_implicit_cg(self, steps):
        """mf_plan_set_implicit_cg: conjugate-gradient steps per row of an implicit ALS solve (0: the direct solve); read at every
        launch, and only under the implicit kind"""
        _check(hip().mf_plan_set_implicit_cg(self._h, int(steps)), "mf_plan_set_implicit_cg")

    def implicit_cg(self):
        """mf_plan_get_implicit_cg: the steps"""
        s = C.c_int()
        _check(hip().mf_plan_get_implicit_cg(self._h, C.byref(s)), "mf_plan_get_implicit_cg")
        return s.value

    def set_als_box(self, sweeps):
        """mf_plan_set_als_box: coordinate-descent sweeps per row of a direct ALS solve, each step exact within the side's box (0:
        Cholesky, then the clamp); read at every launch"""
        _check(hip().mf_plan_set_als_box(self._h, int(sweeps)), "mf_plan_set_als_box")

    def als_box(self):
        """mf_plan_get_als_box: the sweeps"""
        s = C.c_int()
        _check(hip().mf_plan_get_als_box(self._h, C.byref(s)), "mf_plan_get_als_box")
        return s.value

    def als_solve(self, side, other="current"):
        """mf_plan_als_solve: every row of `side` solved against the other side's "current" or "next" buffer, into the side's
        next buffer; only enqueues"""
        _check(hip().mf_plan_als_solve(self._h, SIDES.get(side, side), GENERATIONS.get(other, other)), "mf_plan_als_solve")

    def als_normal(self, side, other, ptr, pitch):
        """mf_plan_als_normal: the normal records of every row of `side` over the plan's own entries, against the other side's
        "current" or "next" buffer, and the Gram record behind them, into the device buffer at `ptr` ((rows + 1) x pitch
        doubles); only enqueues"""
        _check(hip().mf_plan_als_normal(self._h, SIDES.get(side, side), GENERATIONS.get(other, other), ptr, int(pitch)), "mf_plan_als_normal")

    def als_solve_normal(self, side, ptr, pitch):
        """mf_plan_als_solve_normal: every row of `side` solved from the (summed) normal records at `ptr` into the side's next
        buffer; only enqueues"""
        _check(hip().mf_plan_als_solve_normal(self._h, SIDES.get(side, side), ptr, int(pitch)), "mf_plan_als_solve_normal")

    def als_info(self, side):
        """mf_plan_als_info: (solved, kept_empty, kept_not_pd) rows of the side's last solve"""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        _check(hip().mf_plan_als_info(self._h, SIDES.get(side, side), C.byref(a), C.byref(b), C.byref(c)), "mf_plan_als_info")
        return a.value, b.value, c.value

    def set_confidence(self, conf):
        """mf_plan_set_confidence: the scale of the implicit kind's confidences c = 1 + conf * w; read at every launch"""
        _check(hip().mf_plan_set_confidence(self._h, float(conf)), "mf_plan_set_confidence")

    def confidence(self):
        """mf_plan_get_confidence"""
        c = C.c_double()
        _check(hip().mf_plan_get_confidence(self._h, C.byref(c)), "mf_plan_get_confidence")
        return c.value

    def gram(self, side, generation="current", download=True):
        """mf_plan_gram: X^T X over all rows of the side's "current" or "next" buffer as a packed lower triangle (row by row);
        download=False only enqueues and returns None"""
        tri = np.empty(self.feats * (self.feats + 1) // 2, np.float64) if download else None
        _check(hip().mf_plan_gram(self._h, SIDES.get(side, side), GENERATIONS.get(generation, generation),
                                  tri.ctypes.data if download else None), "mf_plan_gram")
        return tri

    def implicit_objective(self):
        """mf_plan_implicit_objective: (all_sq, observed, count) of the current factors"""
        o = ImplicitObjective()
        _check(hip().mf_plan_implicit_objective(self._h, C.byref(o)), "mf_plan_implicit_objective")
        return o.all_sq, o.observed, o.count

    def _side_shape(self, side):
        return (self.items if SIDES[side] == 0 else self.user_count, self.feats)

    def download_adaptive_state(self, side):
        """mf_plan_download_adaptive_state: (m, v, steps, p1, p2) of a side; a side at rest gives zeros, 0, 1.0, 1.0"""
        m, v = np.empty(self._side_shape(side), np.float64), np.empty(self._side_shape(side), np.float64)
        steps, p1, p2 = C.c_int64(), C.c_double(), C.c_double()
        _check(hip().mf_plan_download_adaptive_state(self._h, SIDES[side], m.ctypes.data, v.ctypes.data, C.byref(steps), C.byref(p1),
                                                     C.byref(p2)), "mf_plan_download_adaptive_state")
        return m, v, steps.value, p1.value, p2.value

    def upload_adaptive_state(self, side, m=None, v=None, steps=None, p1=None, p2=None):
        """mf_plan_upload_adaptive_state: what download_adaptive_state returned; None leaves that part as it is"""
        m = None if m is None else np.ascontiguousarray(m, np.float64)
        v = None if v is None else np.ascontiguousarray(v, np.float64)
        assert m is None or m.shape == self._side_shape(side)
        assert v is None or v.shape == self._side_shape(side)
        st = None if steps is None else C.c_int64(int(steps))
        q1 = None if p1 is None else C.c_double(float(p1))
        q2 = None if p2 is None else C.c_double(float(p2))
        _check(hip().mf_plan_upload_adaptive_state(self._h, SIDES[side], None if m is None else m.ctypes.data,
                                                   None if v is None else v.ctypes.data, None if st is None else C.byref(st),
                                                   None if q1 is None else C.byref(q1), None if q2 is None else C.byref(q2)),
               "mf_plan_upload_adaptive_state")

    def penalty(self, rows=False):
        """mf_plan_penalty: (||L_block||^2, ||R||^2) of the current factors; with rows=True also the user_count and the
        items row sums of squares."""
        u, i = C.c_double(), C.c_double()
        ur = np.empty(self.user_count, np.float64) if rows else None
        ir = np.empty(self.items, np.float64) if rows else None
        _check(hip().mf_plan_penalty(self._h, C.byref(u), C.byref(i), ur.ctypes.data if rows else None,
                                     ir.ctypes.data if rows else None), "mf_plan_penalty")
        return (u.value, i.value, ur, ir) if rows else (u.value, i.value)

    def sweep_items(self, seed_from_old=True):
        _check(hip().mf_plan_sweep_items(self._h, 1 if seed_from_old else 0), "mf_plan_sweep_items")

    def sweep_users(self, seed_from_old=True):
        _check(hip().mf_plan_sweep_users_seeded(self._h, 1 if seed_from_old else 0), "mf_plan_sweep_users_seeded")

    def users_next_ptr(self):
        return hip().mf_plan_users_next(self._h)

    def users_current_ptr(self):
        return hip().mf_plan_users_current(self._h)

    def items_next_ptr(self):
        return hip().mf_plan_items_next(self._h)

    def items_current_ptr(self):
        return hip().mf_plan_items_current(self._h)

    def flip(self):
        _check(hip().mf_plan_flip(self._h), "mf_plan_flip")

    def recommend(self):
        best = np.empty(self.user_count, np.int32)
        _check(hip().mf_plan_recommend(self._h, best), "mf_plan_recommend")
        return best

    def recommend_topn(self, n, scores=True):
        """mf_plan_recommend_topn: (items, scores) of shape (user_count, n), or items alone with scores=False."""
        items = np.empty((self.user_count, max(int(n), 0)), np.int32)
        sc = np.empty((self.user_count, max(int(n), 0)), np.float64) if scores else None
        _check(hip().mf_plan_recommend_topn(self._h, int(n), items.ctypes.data, sc.ctypes.data if scores else None),
               "mf_plan_recommend_topn")
        return (items, sc) if scores else items

    def recommend_topn_info(self):
        """(users of the last recommend_topn that went through the exact pass, or -1 when the exact form ran for all;
        form: 0 exact, 1 matrix cores at two workgroups per CU, 2 at one per CU)"""
        n, f = C.c_int64(), C.c_int32()
        _check(hip().mf_plan_recommend_topn_info(self._h, C.byref(n), C.byref(f)), "mf_plan_recommend_topn_info")
        return n.value, f.value

    def similar_items(self, n, metric="cosine", query=None, scores=True):
        """mf_plan_similar_items: the n nearest other items of every query item (all items in ascending order with
        query=None) by "cosine" or "dot" of the rows of the current R: (items, scores) of shape (nq, n), or items alone
        with scores=False."""
        query, qptr, nq = _similar_query(query, self.items)
        items = np.empty((nq, max(int(n), 0)), np.int32)
        sc = np.empty((nq, max(int(n), 0)), np.float64) if scores else None
        _check(hip().mf_plan_similar_items(self._h, int(SIMILAR_METRICS.get(metric, metric)), qptr, nq, int(n),
                                           items.ctypes.data, sc.ctypes.data if scores else None), "mf_plan_similar_items")
        return (items, sc) if scores else items

    def similar_items_info(self):
        """(queries of the last similar_items that went through the exact pass, or -1 when the exact form ran for all;
        form: 0 exact, 1 matrix cores at two workgroups per CU, 2 at one per CU)"""
        n, f = C.c_int64(), C.c_int32()
        _check(hip().mf_plan_similar_items_info(self._h, C.byref(n), C.byref(f)), "mf_plan_similar_items_info")
        return n.value, f.value

    def set_heldout(self, row, col, val):
        """mf_plan_set_heldout: the held-out triples (global user ids); empty arrays remove the set."""
        row = np.ascontiguousarray(row, np.int32)
        col = np.ascontiguousarray(col, np.int32)
        val = np.ascontiguousarray(val, np.float64)
        assert row.shape == col.shape == val.shape and row.ndim == 1
        _check(hip().mf_plan_set_heldout(self._h, int(row.shape[0]), row.ctypes.data, col.ctypes.data, val.ctypes.data),
               "mf_plan_set_heldout")
        self._heldout_n = int(row.shape[0])

    def rank_heldout(self):
        """mf_plan_rank_heldout: the 0-based rank of every held-out entry among its user's unrated items, in the order
        set_heldout was given them (int32; MF_RANK_MASKED for a training pair, MF_RANK_NAN for a NaN score)."""
        rank = np.empty(getattr(self, "_heldout_n", 0), np.int32)
        _check(hip().mf_plan_rank_heldout(self._h, rank.ctypes.data), "mf_plan_rank_heldout")
        return rank

    def rank_heldout_info(self):
        """(entries of the last rank_heldout that went through the exact pass, or -1 when the exact form ran for all;
        form: 0 exact, 1 matrix cores at two workgroups per CU, 2 at one per CU)"""
        n, f = C.c_int64(), C.c_int32()
        _check(hip().mf_plan_rank_heldout_info(self._h, C.byref(n), C.byref(f)), "mf_plan_rank_heldout_info")
        return n.value, f.value

    def loss(self, which="train", rows=False):
        """mf_plan_loss of the training entries ("train") or the held-out set ("heldout"): a Loss (sse, count, rmse); with
        rows=True also the user_count row sums."""
        out = Loss()
        rs = np.empty(self.user_count, np.float64) if rows else None
        code = {"train": MF_LOSS_TRAIN, "heldout": MF_LOSS_HELDOUT}.get(which, which)
        _check(hip().mf_plan_loss(self._h, int(code), C.byref(out), rs.ctypes.data if rows else None), "mf_plan_loss")
        return (out, rs) if rows else out

    def iterate_monitored(self, iters, every=1, tol=0.0):
        """mf_plan_iterate_monitored: (iters_done, [LossPoint, ...])."""
        cap = max(int(iters), 0) // max(int(every), 1) + 2
        trace = (LossPoint * cap)()
        npts, done = C.c_int(), C.c_int()
        _check(hip().mf_plan_iterate_monitored(self._h, int(iters), int(every), float(tol), trace, cap, C.byref(npts),
                                               C.byref(done)), "mf_plan_iterate_monitored")
        return done.value, [trace[i] for i in range(min(npts.value, cap))]

    def recommend_scored(self):
        """Partial scan state per user (CANDIDATE_DTYPE records); item ids relative to this plan's item block."""
        out = np.zeros(self.user_count, CANDIDATE_DTYPE)
        _check(hip().mf_plan_recommend_scored(self._h, out.ctypes.data), "mf_plan_recommend_scored")
        return out

    def recommend_scored_users(self, users):
        """The same for the listed users (local ids) only; record t belongs to users[t]."""
        users = np.ascontiguousarray(users, np.int32)
        out = np.zeros(users.shape[0], CANDIDATE_DTYPE)
        _check(hip().mf_plan_recommend_scored_users(self._h, users, users.shape[0], out.ctypes.data),
               "mf_plan_recommend_scored_users")
        return out

    def recommend_filter(self):
        """Pass 1 alone: (FILTER_DTYPE records, ||L[i]|| per user, max ||R[j]|| over this plan's items)."""
        out = np.zeros(self.user_count, FILTER_DTYPE)
        norm = np.zeros(self.user_count, np.float64)
        rmax = C.c_double()
        _check(hip().mf_plan_recommend_filter(self._h, out.ctypes.data, norm, C.byref(rmax)),
               "mf_plan_recommend_filter")
        return out, norm, rmax.value

    def pitches(self):
        """(users_pitch, items_pitch) of the plan's L and R buffers in doubles."""
        a, b = C.c_int32(), C.c_int32()
        _check(hip().mf_plan_row_pitch(self._h, C.byref(a), C.byref(b)), "mf_plan_row_pitch")
        return a.value, b.value

    def recommend_info(self):
        n = C.c_int64()
        _check(hip().mf_plan_recommend_info(self._h, C.byref(n)), "mf_plan_recommend_info")
        return n.value

    def predict(self):
        B = np.empty((self.user_count, self.items), np.float64)
        _check(hip().mf_plan_predict(self._h, B), "mf_plan_predict")
        return B

    def synchronize(self):
        _check(hip().mf_plan_synchronize(self._h), "mf_plan_synchronize")

    def timing(self, enable=True):
        _check(hip().mf_plan_timing(self._h, 1 if enable else 0), "mf_plan_timing")

    def timing_read(self):
        il, ul = C.c_int64(), C.c_int64()
        ims, ums = C.c_double(), C.c_double()
        _check(hip().mf_plan_timing_read(self._h, C.byref(il), C.byref(ims), C.byref(ul), C.byref(ums)),
               "mf_plan_timing_read")
        return {"item_launches": il.value, "item_ms": ims.value, "user_launches": ul.value, "user_ms": ums.value}

    def describe(self):
        buf = C.create_string_buffer(1024)
        _check(hip().mf_plan_describe(self._h, buf, 1024), "mf_plan_describe")
        return buf.value.decode()
