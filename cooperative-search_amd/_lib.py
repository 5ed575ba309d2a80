"""ctypes binding of libcoopsearch_hip.so (include/coopsearch.h) and the choice between it and torch.ops.coopsearch
(`pick_binding`: either way the package calls one ops object).  No fallback: a missing library raises."""
import ctypes as C
import os
import warnings

import torch

from . import build as _build

ABI_VERSION = 7   # CS_ABI_VERSION of include/coopsearch.h; bumped whenever an export or a struct changes
MT_STRIDE = 672    # CS_MT_STRIDE
MAX_AGENTS = 8
MAX_TARGETS = 16
H_WORDS = 16
# header word indices (enum CS_H_* in coopsearch.h)
H_FOUND, H_NEWLY, H_TARGET_FIND, H_FLAGS, H_TIME_STEP, H_TOTAL_REWARD, H_MT_POS, H_EPISODES = range(8)
H_WORDS_LO, H_WORDS_HI, H_CURR_REWARD, H_NEWLY_RESET = 8, 9, 10, 11
SELECT_SOFTMAX, SELECT_SAMPLE = 1, 2
FREEZE_DONE, AUTO_RESET, ACTIONS_I64, KERNEL_GROUP, KERNEL_LANE, KERNEL_SOLO, KERNEL_DUO, KERNEL_OCT, KERNEL_OD, KERNEL_ODE, KERNEL_LANEV, CHECK_ACTIONS = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048

EXPORTS = ["cs_abi_version", "cs_source_hash", "cs_has_legacy_kernels", "cs_last_error", "cs_state_layout", "cs_init", "cs_seed", "cs_reset", "cs_step",
           "cs_rollout", "cs_rollout_policy", "cs_rollout_policy_flight", "cs_collect_flight", "cs_emit", "cs_snapshot_bytes", "cs_snapshot", "cs_restore", "cs_metrics", "cs_mt_canonical", "cs_mt_advance", "cs_policy_packed_floats", "cs_policy_pack", "cs_policy_pack_device", "cs_policy_forward",
           "cs_policy_conv_features", "cs_policy_conv_features_backward_scratch", "cs_policy_conv_features_backward", "cs_policy_last_error", "cs_store_episodes", "cs_store_episodes_compact", "cs_render_episodes", "cs_coverage_actions", "cs_sweep_episodes", "cs_move_targets", "cs_belief_actions", "cs_plan_actions", "cs_belief_forecast", "cs_plan_forecast_actions", "cs_label_episodes", "cs_grid_features", "cs_feature_episodes", "cs_local_coverage_actions", "cs_local_belief_actions", "cs_local_grid_features", "cs_local_feature_episodes", "cs_local_plan_actions", "cs_local_belief_forecast", "cs_local_plan_forecast_actions", "cs_episodes_last_error", "cs_epsilon_step",
           "cs_gru_seq_forward", "cs_gru_seq_backward", "cs_episode_returns", "cs_gae", "cs_ppo_loss", "cs_bc_loss", "cs_learn_last_error"]


class CsConfig(C.Structure):
    _fields_ = [
        ("variant", C.c_int32), ("n_agents", C.c_int32), ("n_targets", C.c_int32), ("map_size", C.c_int32),
        ("view_range", C.c_int32), ("time_limit", C.c_int32), ("agent_mode", C.c_int32), ("target_mode", C.c_int32),
        ("velocity", C.c_double), ("safe_dist", C.c_double), ("detect_prob", C.c_double),
        ("force_dist", C.c_double), ("force_factor", C.c_double),
        ("cx", C.c_double * MAX_TARGETS), ("cy", C.c_double * MAX_TARGETS),
        ("dx", C.c_double * MAX_TARGETS), ("dy", C.c_double * MAX_TARGETS),
        ("deter", C.c_int32 * MAX_TARGETS),
        ("batch", C.c_int64),
    ]


class CsLayout(C.Structure):
    _fields_ = [("total_bytes", C.c_size_t), ("tgt_off", C.c_size_t), ("agent_off", C.c_size_t),
                ("hdr_off", C.c_size_t), ("mt_off", C.c_size_t), ("ahead_off", C.c_size_t), ("tape_off", C.c_size_t), ("prob_off", C.c_size_t),
                ("job_off", C.c_size_t)]


class CsEpisodeOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("o", "u", "s", "r", "o_next", "s_next", "avail_u", "avail_u_next", "u_onehot",
                                          "padded", "terminated")]


class CsCompactOut(C.Structure):
    """cs_compact_out of include/coopsearch.h: the destinations of the map-once episode keys (replay.COMPACT_KEYS order)."""
    _fields_ = [(k, C.c_void_p) for k in ("map", "s_full", "u", "r", "padded", "terminated")]


class CsRenderParams(C.Structure):
    """cs_render_params of include/coopsearch.h: what cs_render_episodes draws (render.RenderSpec computes the radii)."""
    _fields_ = [(k, C.c_int32) for k in ("n_agents", "n_targets", "state_width", "size", "side", "map_width", "rv", "rt", "rtr",
                                         "tri_len", "layers", "reserved")] + \
               [(k, C.c_uint8 * 4) for k in ("background", "sensor_tint", "sensor_ring", "target", "target_found", "bar_on",
                                             "bar_off")] + [("palette_dev", C.c_void_p), ("lut_dev", C.c_void_p)]


class CsCoverageParams(C.Structure):
    """cs_coverage_params of include/coopsearch.h: the greedy coverage baseline (baseline.CoverageAgents computes the fields)."""
    _fields_ = [(k, C.c_int32) for k in ("n_agents", "side", "view_range", "keep", "regrow", "lookahead", "state_width", "reserved")]


class CsSweepParams(C.Structure):
    """cs_sweep_params of include/coopsearch.h: swept-area accounting of recorded episodes (sweep.sweep_episodes fills the fields)."""
    _fields_ = [(k, C.c_int32) for k in ("n_agents", "side", "view_range", "state_width", "rows", "reserved")]


class CsMotionParams(C.Structure):
    """cs_motion_params of include/coopsearch.h: one move of the unfound targets (motion.TargetMotion holds the fields)."""
    _fields_ = [("mode", C.c_int32), ("persist", C.c_int32), ("seed", C.c_uint32), ("reserved", C.c_int32), ("speed", C.c_double),
                ("sense", C.c_double), ("env_offset", C.c_int64)]


class CsBeliefParams(C.Structure):
    """cs_belief_params of include/coopsearch.h: the target-density filter policy (belief.BeliefAgents computes the fields)."""
    _fields_ = [(k, C.c_int32) for k in ("n_agents", "side", "view_range", "keep", "lookahead", "state_width", "mode", "moved", "sense16")] + \
               [("dx", C.c_int32 * 16), ("dy", C.c_int32 * 16), ("reserved", C.c_int32)]


class CsPlanParams(C.Structure):
    """cs_plan_params of include/coopsearch.h: the receding-horizon planner (plan.PlanAgents holds the fields)."""
    _fields_ = [(k, C.c_int32) for k in ("n_agents", "side", "view_range", "depth", "stride", "discount", "state_width", "reserved")]


class CsForecastParams(C.Structure):
    """cs_forecast_params of include/coopsearch.h: the density along the planning horizon (forecast.ForecastAgents computes the fields)."""
    _fields_ = [(k, C.c_int32) for k in ("n_agents", "side", "levels", "mode", "sense16")] + \
               [("dx", C.c_int32 * 16), ("dy", C.c_int32 * 16), ("moves", C.c_int32 * 5), ("reserved", C.c_int32)]


class CsLabelParams(C.Structure):
    """cs_label_params of include/coopsearch.h: an expert relabels recorded episodes (imitate.expert_params computes the fields)."""
    _fields_ = [(k, C.c_int32) for k in ("expert", "n_agents", "side", "view_range", "keep", "regrow", "lookahead", "state_width", "mode",
                                         "sense16", "every", "moving")] + \
               [("dx", C.c_int32 * 16), ("dy", C.c_int32 * 16), ("reserved", C.c_int32)]


class CsGridParams(C.Structure):
    """cs_grid_params of include/coopsearch.h: the grid observations of one decision (gridobs.grid_features fills the fields)."""
    _fields_ = [(k, C.c_int32) for k in ("n_agents", "side", "view_range", "lookahead", "state_width", "reserved")]


class CsLocalParams(C.Structure):
    """cs_local_params of include/coopsearch.h: coverage under a communication range (local.LocalCoverageAgents computes the fields)."""
    _fields_ = [(k, C.c_int32) for k in ("n_agents", "side", "view_range", "keep", "regrow", "lookahead", "state_width", "comm_range",
                                         "reserved")]


class CsLocalBeliefParams(C.Structure):
    """cs_local_belief_params of include/coopsearch.h: the density filter under a communication range (local_belief.LocalBeliefAgents
    computes the fields)."""
    _fields_ = [(k, C.c_int32) for k in ("n_agents", "side", "view_range", "keep", "lookahead", "state_width", "mode", "moved", "sense16")] + \
               [("dx", C.c_int32 * 16), ("dy", C.c_int32 * 16), ("comm_range", C.c_int32), ("reserved", C.c_int32)]


class CsLocalLabelParams(C.Structure):
    """cs_local_label_params of include/coopsearch.h: a local filter walks recorded episodes (localobs.local_expert_params computes the
    fields): cs_label_params' fields, then comm_range and reserved."""
    _fields_ = CsLabelParams._fields_[:-1] + [("comm_range", C.c_int32), ("reserved", C.c_int32)]


class CsLocalPlanParams(C.Structure):
    """cs_local_plan_params of include/coopsearch.h: the planner on private grids under a communication range
    (local_plan.LocalPlanAgents holds the fields): cs_plan_params' fields, then comm_range and reserved."""
    _fields_ = CsPlanParams._fields_[:-1] + [("comm_range", C.c_int32), ("reserved", C.c_int32)]


class CsEpsilon(C.Structure):
    """cs_epsilon of include/coopsearch.h: the exploration schedule of common/rollout.py:35-41,75-76,133-135."""
    _fields_ = [("epsilon", C.c_double), ("anneal", C.c_double), ("min_epsilon", C.c_double), ("per_step", C.c_int32),
                ("reserved", C.c_int32), ("eps_dev", C.c_void_p), ("trace_dev", C.c_void_p)]


class CoopSearchError(RuntimeError):
    pass


_lib = None


def library_path():
    return _build.LIB_PATH


def load():
    """Load (building first if the in-tree .so is missing or was built from other sources).  Staleness is decided by the
    source hash recorded at build time (build.source_hash), not by mtimes; where hipcc is absent a library whose recorded
    hash differs is still loaded -- with a warning -- as long as its ABI version matches (checked below)."""
    global _lib
    if _lib is not None:
        return _lib
    path = _build.LIB_PATH
    if _build.is_stale():
        if _build.hipcc_path() is None:
            if not os.path.exists(path):
                raise CoopSearchError(
                    f"{path} is missing and hipcc is not available: the HIP extension is required (no CPU fallback)")
            warnings.warn(f"{path} was not built from the sources present here (recorded source hash "
                          f"{_build._recorded_hash(path)!r}, sources {_build.source_hash()!r}) and hipcc is not available to "
                          "rebuild it: loading it as it is (the ABI version is checked)", RuntimeWarning, stacklevel=2)
        else:
            _build.build_extension()
    L = C.CDLL(path)
    vp = C.c_void_p
    L.cs_abi_version.restype = C.c_int
    L.cs_last_error.restype = C.c_char_p
    if hasattr(L, "cs_source_hash"):
        L.cs_source_hash.restype = C.c_char_p
    L.cs_state_layout.argtypes = [C.POINTER(CsConfig), C.POINTER(CsLayout)]
    L.cs_init.argtypes = [C.POINTER(CsConfig), vp, vp]
    L.cs_seed.argtypes = [C.POINTER(CsConfig), vp, vp, vp]
    L.cs_reset.argtypes = [C.POINTER(CsConfig), vp, vp, C.c_int, vp, vp, vp]
    L.cs_step.argtypes = [C.POINTER(CsConfig), vp, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    L.cs_rollout.argtypes = [C.POINTER(CsConfig), vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
    L.cs_rollout_policy.argtypes = [C.POINTER(CsConfig), vp, vp, vp, vp, C.c_int, C.c_int, C.POINTER(CsEpsilon), C.c_uint64, C.c_uint32,
                                    C.c_uint64, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.cs_rollout_policy_flight.argtypes = [C.POINTER(CsConfig)] + [vp] * 11 + [C.c_int, C.c_int, C.POINTER(CsEpsilon), C.c_uint64, C.c_uint32,
                                           C.c_uint64, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.cs_collect_flight.argtypes = L.cs_rollout_policy_flight.argtypes   # map / state tables in place of obs / state_out
    L.cs_epsilon_step.argtypes = [C.POINTER(CsConfig), vp, C.c_int, vp, C.c_double, C.c_double, vp, vp]
    L.cs_emit.argtypes = [C.POINTER(CsConfig), vp, vp, vp, vp]
    L.cs_metrics.argtypes = [C.POINTER(CsConfig), vp, vp, vp]
    L.cs_snapshot_bytes.argtypes = [C.POINTER(CsConfig)]
    L.cs_snapshot_bytes.restype = C.c_size_t
    L.cs_snapshot.argtypes = [C.POINTER(CsConfig), vp, vp, C.c_int64, vp, vp]
    L.cs_restore.argtypes = [C.POINTER(CsConfig), vp, vp, C.c_int64, vp, vp, C.c_int64, vp, vp, vp, vp]
    L.cs_mt_canonical.argtypes = [C.POINTER(CsConfig), vp, vp, vp]
    L.cs_mt_advance.argtypes = [C.POINTER(CsConfig), vp, C.c_int, vp]
    L.cs_policy_packed_floats.restype = C.c_size_t
    L.cs_policy_last_error.restype = C.c_char_p
    L.cs_episodes_last_error.restype = C.c_char_p
    L.cs_store_episodes.argtypes = [C.c_int] * 6 + [vp] * 6 + [C.POINTER(CsEpisodeOut), vp]
    L.cs_store_episodes_compact.argtypes = [C.c_int] * 5 + [vp] * 6 + [C.POINTER(CsCompactOut), vp]
    L.cs_render_episodes.argtypes = [C.POINTER(CsRenderParams), vp, vp, vp, C.c_int, C.c_int, vp, vp]
    L.cs_coverage_actions.argtypes = [C.POINTER(CsCoverageParams), vp, C.c_int, vp, vp, vp]
    L.cs_sweep_episodes.argtypes = [C.POINTER(CsSweepParams), vp, vp, C.c_int, vp, vp, vp, vp]
    L.cs_move_targets.argtypes = [C.POINTER(CsConfig), vp, C.POINTER(CsMotionParams), vp]
    L.cs_belief_actions.argtypes = [C.POINTER(CsBeliefParams), vp, C.c_int, vp, vp, vp, vp]
    L.cs_plan_actions.argtypes = [C.POINTER(CsPlanParams), vp, C.c_int, vp, vp, vp, vp, vp]
    L.cs_belief_forecast.argtypes = [C.POINTER(CsForecastParams), vp, vp, C.c_int, vp, vp]
    L.cs_plan_forecast_actions.argtypes = [C.POINTER(CsPlanParams), vp, C.c_int, vp, vp, vp, vp, vp]
    L.cs_label_episodes.argtypes = [C.POINTER(CsLabelParams), vp, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    L.cs_grid_features.argtypes = [C.POINTER(CsGridParams), vp, C.c_int, vp, vp, vp]
    L.cs_feature_episodes.argtypes = [C.POINTER(CsLabelParams), vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
    L.cs_local_coverage_actions.argtypes = [C.POINTER(CsLocalParams), vp, C.c_int, vp, vp, vp]
    L.cs_local_belief_actions.argtypes = [C.POINTER(CsLocalBeliefParams), vp, C.c_int, vp, vp, vp, vp, vp]
    L.cs_local_grid_features.argtypes = [C.POINTER(CsGridParams), vp, C.c_int, vp, vp, vp]
    L.cs_local_feature_episodes.argtypes = [C.POINTER(CsLocalLabelParams), vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
    L.cs_local_plan_actions.argtypes = [C.POINTER(CsLocalPlanParams), vp, C.c_int, vp, vp, vp, vp, vp]
    L.cs_local_belief_forecast.argtypes = [C.POINTER(CsForecastParams), vp, vp, vp, C.c_int, vp, vp]
    L.cs_local_plan_forecast_actions.argtypes = [C.POINTER(CsLocalPlanParams), vp, C.c_int, vp, vp, vp, vp, vp]
    L.cs_bc_loss.argtypes = [vp] * 4 + [C.c_int64, C.c_int, C.c_int] + [vp] * 4 + [C.c_int64, vp]
    L.cs_policy_pack.argtypes = [vp] * 10 + [C.c_int, C.c_int, vp]
    L.cs_policy_pack_device.argtypes = [vp] * 10 + [C.c_int, C.c_int, vp, vp, vp]
    L.cs_policy_forward.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int,
                                    C.c_float, vp, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, vp]
    L.cs_policy_conv_features.argtypes = [vp] * 7 + [C.c_int64, C.c_int, vp, vp]
    L.cs_policy_conv_features_backward_scratch.argtypes = [C.c_int, C.POINTER(C.c_int64)]
    L.cs_policy_conv_features_backward.argtypes = [vp] * 7 + [C.c_int64, C.c_int] + [vp] * 8 + [C.c_int64, vp]
    L.cs_learn_last_error.restype = C.c_char_p
    L.cs_gru_seq_forward.argtypes = [vp] * 4 + [C.c_int, C.c_int, vp, vp, vp]
    L.cs_gru_seq_backward.argtypes = [vp] * 5 + [C.c_int, C.c_int, vp, vp, vp, vp]
    L.cs_episode_returns.argtypes = [vp] * 4 + [C.c_int, C.c_int, C.c_float, C.c_float, vp, vp]
    L.cs_gae.argtypes = [vp] * 5 + [C.c_int, C.c_int, C.c_float, C.c_float, vp, vp, vp]
    L.cs_ppo_loss.argtypes = [vp] * 6 + [C.c_int64, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float] + [vp] * 6 + [C.c_int64, vp]
    for name in EXPORTS:
        fn = getattr(L, name)
        if name not in ("cs_abi_version", "cs_source_hash", "cs_has_legacy_kernels", "cs_last_error", "cs_policy_packed_floats", "cs_snapshot_bytes", "cs_policy_last_error",
                        "cs_episodes_last_error", "cs_learn_last_error"):
            fn.restype = C.c_int
    if L.cs_abi_version() != ABI_VERSION:
        raise CoopSearchError(f"{path}: ABI version {L.cs_abi_version()}, this package binds version {ABI_VERSION} "
                              "(stale library: rebuild with `python -m cooperative_search_amd.build`)")
    # The hash COMPILED INTO the library is the truth about what it was built from (the .srchash sidecar above is only the
    # shortcut that decides about a rebuild before anything is dlopen'ed; a copied .so can carry a wrong or no sidecar).  The ABI
    # version guards exports and structs only -- kernels change behaviour without touching either -- so a library of other sources
    # is an error under COOPSEARCH_STRICT=1 (tests, CI) and a warning naming both hashes otherwise.  COOPSEARCH_LIB (experimental
    # one-team-size builds) opts out.
    if os.environ.get("COOPSEARCH_LIB"):
        # a variant build says what it should have been compiled from (build.variant_hash: sources AND flags) through
        # COOPSEARCH_LIB_HASH; without that variable the opt-out stands (ad-hoc experiments)
        want = os.environ.get("COOPSEARCH_LIB_HASH")
        built = L.cs_source_hash().decode() if hasattr(L, "cs_source_hash") else ""
        if want and built != want:
            raise CoopSearchError(f"{path} carries source hash {built!r}, expected {want!r}: a stale variant build "
                                  "(rebuild it: cooperative_search_amd.build.build_variant)")
    else:
        built = L.cs_source_hash().decode() if hasattr(L, "cs_source_hash") else ""
        want = _build.source_hash()
        if built != want:
            msg = (f"{path} was built from sources with hash {built!r}, the sources present here hash to {want!r}: "
                   "kernels may behave differently from what the tests restate (rebuild with `python -m cooperative_search_amd.build`)")
            if os.environ.get("COOPSEARCH_STRICT") == "1":
                raise CoopSearchError(msg)
            warnings.warn(msg, RuntimeWarning, stacklevel=2)
    _lib = L
    return L


_ops = None


def torch_ops():
    """torch.ops.coopsearch (csrc/torch_ops.cpp): tensor-level ops over the same C ABI -- device / dtype / contiguity
    checks in C++ (TORCH_CHECK), stream = torch's current HIP stream, the tensors' device made current.  Builds
    coopsearch_torch.so (g++: host code only) first when it is missing or was built from other sources; raises when it can
    neither be built nor loaded -- `pick_binding` turns that into the ctypes route for callers that did not ask for torch."""
    global _ops
    if _ops is not None:
        return _ops
    load()   # libcoopsearch_hip.so first: coopsearch_torch.so links it
    if _build.torch_ops_stale():
        if _build.cxx_path() is None:
            if not os.path.exists(_build.TORCH_LIB_PATH):
                raise CoopSearchError(f"{_build.TORCH_LIB_PATH} is missing and there is no g++ to build it")
            warnings.warn(f"{_build.TORCH_LIB_PATH} was not built from the torch_ops.cpp present here and there is no g++ "
                          "to rebuild it: loading it as it is (the ABI version is checked)", RuntimeWarning, stacklevel=2)
        else:
            _build.build_torch_ops()
    torch.ops.load_library(_build.TORCH_LIB_PATH)
    if int(torch.ops.coopsearch.abi_version()) != ABI_VERSION:
        raise CoopSearchError(f"{_build.TORCH_LIB_PATH}: ABI version mismatch (stale library)")
    _ops = torch.ops.coopsearch
    return _ops


def torch_ops_for(what):
    """`torch_ops()` for a caller that has no other route to its kernels: whatever keeps the op layer from loading (no compiler, no
    torch headers, a dlopen failure) becomes a CoopSearchError that starts with `what`, e.g. "the coverage kernel needs"."""
    try:
        return torch_ops()
    except CoopSearchError:
        raise
    except Exception as exc:   # noqa: BLE001
        raise CoopSearchError(f"{what} torch.ops.coopsearch, which is unavailable ({type(exc).__name__}: {exc})") from exc


def _cfg(cfg):
    """The cs_config whose bytes the CPU uint8 tensor `cfg` holds (what the ops take; BatchedFlightEnv._cfg_t), in place."""
    return CsConfig.from_address(cfg.data_ptr())


def _p(t):
    return None if t is None else t.data_ptr()


def _epsilon(epsilon, eps_env, anneal, min_epsilon, per_step, eps_trace):
    return CsEpsilon(epsilon, anneal, min_epsilon, 1 if per_step else 0, 0, _p(eps_env), _p(eps_trace))


def _action_flags(cfg, actions, flags):
    """action_flags of csrc/torch_ops.cpp: ACTIONS_I64 from the dtype; CHECK_ACTIONS as the caller decided (CHECK_ACTIONS = on,
    OP_NO_CHECK_ACTIONS = off, a bit that never reaches the C ABI), else check_actions_default(batch)."""
    if flags & (CHECK_ACTIONS | OP_NO_CHECK_ACTIONS):
        on = not flags & OP_NO_CHECK_ACTIONS
    else:
        on = check_actions_default(_cfg(cfg).batch)
    return (flags & ~(ACTIONS_I64 | CHECK_ACTIONS | OP_NO_CHECK_ACTIONS)) | (ACTIONS_I64 if actions.dtype == torch.int64 else 0) \
        | (CHECK_ACTIONS if on else 0)


class CtypesOps:
    """The ctypes twin of torch.ops.coopsearch: the ops the package calls, under the same names and with the same arguments
    (tests/test_capi_cpu.py holds the two together), straight to the C ABI.  A method makes its tensors' device current, takes
    torch's current stream on it, turns tensors into pointers and raises from the entry point's `*_last_error`; it checks no
    tensor -- the op layer's TORCH_CHECKs have no counterpart here."""

    def __init__(self):
        self._L = load()

    def _launch(self, on, fn, *args, error=None):
        """fn(*args, stream): the cs_* entry points launch on the process's current device, so `on`'s device is made current
        for the call (the ops do the same in C++ with a HIPGuard); an env on cuda:1 works while cuda:0 is current."""
        with torch.cuda.device(on.device):
            rc = fn(*args, torch.cuda.current_stream(on.device).cuda_stream)
        if error is None:
            check(rc)
        elif rc != 0:
            raise CoopSearchError(error().decode())

    def _env(self, fn, cfg, state, *args):
        self._launch(state, fn, _cfg(cfg), state.data_ptr(), *args)

    def _policy(self, on, fn, *args):
        self._launch(on, fn, *args, error=self._L.cs_policy_last_error)

    def state_bytes(self, cfg):
        lay = CsLayout()
        check(self._L.cs_state_layout(_cfg(cfg), C.byref(lay)))
        return lay.total_bytes

    def env_init(self, cfg, state):
        self._env(self._L.cs_init, cfg, state)

    def env_seed(self, cfg, state, seeds):
        self._env(self._L.cs_seed, cfg, state, _p(seeds))

    def env_reset(self, cfg, state, mask, init, obs, state_out):
        self._env(self._L.cs_reset, cfg, state, _p(mask), 1 if init else 0, _p(obs), _p(state_out))

    def env_step(self, cfg, state, actions, flags, reward, terminated, win, obs, state_out):
        self._env(self._L.cs_step, cfg, state, _p(actions), _action_flags(cfg, actions, flags), _p(reward), _p(terminated), _p(win),
                  _p(obs), _p(state_out))

    def env_rollout(self, cfg, state, actions, flags, reward, terminated, win, obs, state_out):
        self._env(self._L.cs_rollout, cfg, state, _p(actions), actions.shape[0], _action_flags(cfg, actions, flags), _p(reward),
                  _p(terminated), _p(win), _p(obs), _p(state_out))

    def env_emit(self, cfg, state, obs, state_out):
        self._env(self._L.cs_emit, cfg, state, _p(obs), _p(state_out))

    def env_metrics(self, cfg, state, out4):
        self._env(self._L.cs_metrics, cfg, state, _p(out4))

    def mt_advance(self, cfg, state, min_ahead):
        self._env(self._L.cs_mt_advance, cfg, state, min_ahead)

    def mt_canonical(self, cfg, state, rows_out):
        self._env(self._L.cs_mt_canonical, cfg, state, _p(rows_out))

    def epsilon_step(self, cfg, state, flags, eps_env, anneal, min_epsilon, trace_row):
        self._env(self._L.cs_epsilon_step, cfg, state, flags, _p(eps_env), anneal, min_epsilon, _p(trace_row))

    def policy_forward(self, packed, obs, obs_stride, obs_offset, last, feat, rows_per_feat, hidden, q, actions, rows, n_agents,
                       n_actions, epsilon, eps_env, seed, step, row0, select):
        self._policy(packed, self._L.cs_policy_forward, _p(packed), _p(obs), obs_stride, obs_offset, _p(last), _p(feat),
                     rows_per_feat, _p(hidden), _p(q), _p(actions), rows, n_agents, n_actions, epsilon, _p(eps_env), seed, step, row0,
                     select)

    def policy_conv_features(self, conv1_w, conv1_b, conv2_w, conv2_b, lin_w, lin_b, maps, map_stride, n_maps, feat):
        self._policy(maps, self._L.cs_policy_conv_features, _p(conv1_w), _p(conv1_b), _p(conv2_w), _p(conv2_b), _p(lin_w), _p(lin_b),
                     _p(maps), map_stride, n_maps, _p(feat))

    def policy_pack_device(self, fc1_w, fc1_b, w_ih, b_ih, w_hh, b_hh, fc2a_w, fc2a_b, fc2b_w, fc2b_b, packed, status):
        ws = (fc1_w, fc1_b, w_ih, b_ih, w_hh, b_hh, fc2a_w, fc2a_b, fc2b_w, fc2b_b)
        self._policy(packed, self._L.cs_policy_pack_device, *map(_p, ws), fc1_w.shape[1], fc2b_w.shape[0], _p(packed), _p(status))

    def _closed_loop(self, fn, cfg, state, ins, T, flags, eps, seed, step0, row0, select, outs):
        self._env(fn, cfg, state, *map(_p, ins), T, flags, C.byref(eps), seed, step0, row0, select, *map(_p, outs))

    def rollout_policy(self, cfg, state, packed, hidden, last, T, flags, epsilon, eps_env, anneal, min_epsilon, per_step, eps_trace,
                       seed, step0, row0, select, actions, reward, terminated, win, obs, state_out):
        self._closed_loop(self._L.cs_rollout_policy, cfg, state, (packed, hidden, last), T, flags,
                          _epsilon(epsilon, eps_env, anneal, min_epsilon, per_step, eps_trace), seed, step0, row0, select,
                          (actions, reward, terminated, win, obs, state_out))

    def rollout_policy_flight(self, cfg, state, packed, c1w, c1b, c2w, c2b, lw, lb, hidden, last, scratch, T, flags, epsilon, eps_env,
                              anneal, min_epsilon, per_step, eps_trace, seed, step0, row0, select, actions, reward, terminated, win,
                              obs, state_out):
        self._closed_loop(self._L.cs_rollout_policy_flight, cfg, state, (packed, c1w, c1b, c2w, c2b, lw, lb, hidden, last, scratch),
                          T, flags, _epsilon(epsilon, eps_env, anneal, min_epsilon, per_step, eps_trace), seed, step0, row0, select,
                          (actions, reward, terminated, win, obs, state_out))

    def collect_flight(self, cfg, state, packed, c1w, c1b, c2w, c2b, lw, lb, hidden, last, scratch, T, flags, epsilon, eps_env,
                       anneal, min_epsilon, per_step, eps_trace, seed, step0, row0, select, actions, reward, terminated, win,
                       map_tab, state_tab):
        self._closed_loop(self._L.cs_collect_flight, cfg, state, (packed, c1w, c1b, c2w, c2b, lw, lb, hidden, last, scratch),
                          T, flags, _epsilon(epsilon, eps_env, anneal, min_epsilon, per_step, eps_trace), seed, step0, row0, select,
                          (actions, reward, terminated, win, map_tab, state_tab))

    def store_episodes(self, o_tab, s_tab, u_tab, r_tab, term_tab, slots, n_actions, outs):
        T, B, n = u_tab.shape
        eo = CsEpisodeOut(*map(_p, outs))
        self._launch(o_tab, self._L.cs_store_episodes, B, T, n, n_actions, o_tab.shape[-1], s_tab.shape[-1], _p(o_tab), _p(s_tab),
                     _p(u_tab), _p(r_tab), _p(term_tab), _p(slots), C.byref(eo), error=self._L.cs_episodes_last_error)

    def store_episodes_compact(self, map_tab, s_tab, u_tab, r_tab, term_tab, slots, outs):
        T, B, n = u_tab.shape
        if any(t.shape[1] != (T + 1 if k < 2 else T) for k, t in enumerate(outs)):   # map and s_full come first (CsCompactOut)
            raise ValueError("assemble_episodes_compact: destinations must be [slots, T (+ 1), ...]")
        co = CsCompactOut(*map(_p, outs))
        self._launch(map_tab, self._L.cs_store_episodes_compact, B, T, n, map_tab.shape[-1], s_tab.shape[-1], _p(map_tab),
                     _p(s_tab), _p(u_tab), _p(r_tab), _p(term_tab), _p(slots), C.byref(co), error=self._L.cs_episodes_last_error)


_ctypes_ops = None


def ctypes_ops():
    global _ctypes_ops
    if _ctypes_ops is None:
        _ctypes_ops = CtypesOps()
    return _ctypes_ops


def pick_binding(binding=None):
    """'torch' | 'ctypes' | None -> (name, ops): torch.ops.coopsearch or its ctypes twin (`CtypesOps`), never None.  None = the
    torch op layer when it can be built / loaded, else the ctypes route with a warning (same library, same kernels); an
    experimental library (COOPSEARCH_LIB) is only reachable through ctypes.  An explicit 'torch' raises when the op library is
    unavailable."""
    if binding not in (None, "torch", "ctypes"):
        raise ValueError("binding must be 'torch' (torch.ops.coopsearch, csrc/torch_ops.cpp) or 'ctypes'")
    if binding == "ctypes" or (binding is None and os.environ.get("COOPSEARCH_LIB")):
        return "ctypes", ctypes_ops()
    try:
        return "torch", torch_ops()
    except Exception as exc:   # noqa: BLE001 -- compiler missing, torch headers missing, dlopen failure, ABI mismatch
        if binding == "torch":
            raise
        warnings.warn(f"torch.ops.coopsearch is unavailable ({type(exc).__name__}: {exc}); using the ctypes binding of the "
                      "same library", RuntimeWarning, stacklevel=3)
        return "ctypes", ctypes_ops()


def has_legacy_kernels():
    """cs_has_legacy_kernels() of the loaded library: False since round 6 (the 16-lane rollout kernels of rounds 1-2 were removed; the
    entry point stays for ABI 7)."""
    L = load()
    L.cs_has_legacy_kernels.restype = C.c_int
    return bool(L.cs_has_legacy_kernels())


OP_NO_CHECK_ACTIONS = 1 << 30   # torch op layer only (csrc/torch_ops.cpp): 'the caller decided: no check'; never reaches the C ABI


def check(rc):
    if rc != 0:
        msg = load().cs_last_error().decode()
        if msg.startswith("list index out of range"):   # CS_CHECK_ACTIONS: the reference's IndexError (dyaw[act], flight_env_easy.py:262)
            raise IndexError(msg)
        raise CoopSearchError(f"coopsearch error {rc}: {msg}")


def check_actions_default(batch):
    """CS_CHECK_ACTIONS is on by default for batches of up to 64 envs; COOPSEARCH_CHECK_ACTIONS=0 / 1 forces it off / on
    (same rule as csrc/torch_ops.cpp:check_actions_default)."""
    e = os.environ.get("COOPSEARCH_CHECK_ACTIONS", "")
    return batch <= 64 if e == "" else e[0] != "0"
