"""ctypes binding of libbcmpc.so (include/bcmpc.h).

The library is built in-tree (``make`` / ``__graft_entry__.build()``) and is
the only compute path: if it is missing this module raises ImportError --
there is no CPU fallback.

PyTorch-ROCm ships its own ``libamdhip64.so.7`` (same SONAME as
/opt/rocm's).  Importing torch first makes the dynamic linker reuse torch's
HIP runtime for libbcmpc, so device pointers from torch tensors and from the
engine live in ONE runtime.
"""
from __future__ import annotations

import ctypes
import os

try:  # single HIP runtime per process (see module docstring)
    import torch  # noqa: F401
except Exception:  # pragma: no cover - torch is part of the image
    torch = None

LIB_PATH = os.environ.get("BCMPC_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libbcmpc.so")

MAX_LAYERS = 8
MAX_STATE = 32
MAX_ACTION = 16
COMM_ID_BYTES = 128
ABI_VERSION = 5

OK, ERR_ARG, ERR_UNSUPPORTED, ERR_HIP, ERR_STATE, ERR_EMPTY = range(6)
ACT_TANH, ACT_RELU = 0, 1
COST_CHEETAH, COST_NONE, COST_REWARD, COST_TERMS = 0, 1, 2, 3
MAX_COST_TERMS = 32
TERM_THRESHOLD, TERM_DIFF, TERM_LINEAR, TERM_QUADRATIC = range(4)
TERM_RATE = 4               # bcmpc_cost_term_x alone (bcmpc_set_cost_terms_x)
MAX_REF_CHANNELS = 16
SRC_STATE, SRC_NEXT_STATE, SRC_ACTION = range(3)
CMP_GE, CMP_GT, CMP_LE, CMP_LT = range(4)
MAX_MEMBERS = 16
ENSEMBLE_MEAN, ENSEMBLE_MEAN_STD, ENSEMBLE_WORST = range(3)
ENSEMBLE_RULES = {"mean": ENSEMBLE_MEAN, "mean_std": ENSEMBLE_MEAN_STD, "worst": ENSEMBLE_WORST}
MODEL_DELTA, MODEL_REWARD = 0, 1
PREC_FP32, PREC_SPLIT_F16, PREC_F16 = 0, 1, 2
# "f16": single-pass f16 MFMA (BASELINE cfg3's bf16-class GEMM), not the fp32 tolerance
PRECISIONS = {"fp32": PREC_FP32, "split": PREC_SPLIT_F16, "f16": PREC_F16}
KERNELS = {"auto": 0, "solo": 1, "group2": 2, "group4": 3, "group8": 4, "split1": 5, "split2": 6, "split4": 7, "splitr": 8, "team": 9}
# ("splitr" and "group2" stay in the enum for the ABI; bcmpc_create refuses them since round 6)


class Config(ctypes.Structure):
    _fields_ = [
        ("state_dim", ctypes.c_int32),
        ("action_dim", ctypes.c_int32),
        ("hidden", ctypes.c_int32),
        ("n_layers", ctypes.c_int32),
        ("activation", ctypes.c_int32),
        ("layer_norm", ctypes.c_int32),
        ("horizon", ctypes.c_int32),
        ("cost", ctypes.c_int32),
        ("num_paths", ctypes.c_int64),
        ("precision", ctypes.c_int32),
        ("device", ctypes.c_int32),
        ("kernel", ctypes.c_int32),
        ("policy_hidden", ctypes.c_int32),
        ("policy_layers", ctypes.c_int32),
        ("policy_mode", ctypes.c_int32),
        ("model", ctypes.c_int32),
        ("reserved", ctypes.c_int32 * 3),
    ]


_FP = ctypes.POINTER(ctypes.c_float)
_DP = ctypes.POINTER(ctypes.c_double)


class Weights(ctypes.Structure):
    _fields_ = [
        ("kernels", ctypes.POINTER(_FP)),
        ("biases", ctypes.POINTER(_FP)),
        ("ln_gamma", ctypes.POINTER(_FP)),
        ("ln_beta", ctypes.POINTER(_FP)),
        ("mean_obs", _DP),
        ("std_obs", _DP),
        ("mean_action", _DP),
        ("std_action", _DP),
        ("mean_deltas", _DP),
        ("std_deltas", _DP),
        ("mean_reward", _DP),
        ("std_reward", _DP),
    ]


class Policy(ctypes.Structure):
    _fields_ = [
        ("kernels", ctypes.POINTER(_FP)),
        ("biases", ctypes.POINTER(_FP)),
        ("ob_mean", _FP),
        ("ob_std", _FP),
        ("logstd", _FP),
        ("explore", ctypes.c_double),
    ]


POLICY_MODES = {"explore": 0, "stochastic": 1}

VALUE_MAX_LAYERS, VALUE_MAX_HIDDEN = 4, 256


class ValueNet(ctypes.Structure):
    """bcmpc_value_net: the critic of a terminal value (bc_mpc_amd/value.py ValueSpec)."""
    _fields_ = [
        ("kernels", ctypes.POINTER(_FP)),
        ("biases", ctypes.POINTER(_FP)),
        ("ob_mean", _FP),
        ("ob_std", _FP),
        ("n_layers", ctypes.c_int32),
        ("hidden", ctypes.c_int32),
        ("state_dim", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class Cem(ctypes.Structure):
    _fields_ = [
        ("iterations", ctypes.c_int32),
        ("n_elite", ctypes.c_int32),
        ("alpha", ctypes.c_double),
        ("k_global", ctypes.c_int64),
    ]


class CostTerm(ctypes.Structure):
    """bcmpc_cost_term (32 bytes): one term of a declarative cost (cost_functions.TermCost)."""
    _fields_ = [
        ("kind", ctypes.c_int32),
        ("source", ctypes.c_int32),
        ("index", ctypes.c_int32),
        ("cmp", ctypes.c_int32),
        ("weight", ctypes.c_double),
        ("param", ctypes.c_double),
    ]


class CostTermX(ctypes.Structure):
    """bcmpc_cost_term_x (48 bytes): a term that may name a reference channel (``ref``, -1: none) or be a RATE."""
    _fields_ = CostTerm._fields_ + [
        ("ref", ctypes.c_int32),
        ("reserved", ctypes.c_int32 * 3),
    ]


class Elite(ctypes.Structure):
    _fields_ = [("cost", ctypes.c_double), ("index", ctypes.c_int64)]


class Mppi(ctypes.Structure):
    _fields_ = [
        ("iterations", ctypes.c_int32),
        ("lambda_", ctypes.c_double),          # bcmpc_mppi.lambda (the temperature)
        ("k_global", ctypes.c_int64),
    ]


class Sampling(ctypes.Structure):
    """bcmpc_sampling: the planners' sampling distribution (bc_mpc_amd/sampling.py); zeros are the default."""
    _fields_ = [
        ("rho", ctypes.c_double),
        ("keep_elites", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class MppiExt(ctypes.Structure):
    """bcmpc_mppi_ext (40 bytes): MPPI's control-cost weight and sigma update (bc_mpc_amd/mppi_update.py)."""
    _fields_ = [
        ("control_weight", ctypes.c_double),
        ("adapt_sigma", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("sigma_alpha", ctypes.c_double),
        ("min_std", ctypes.c_double),
        ("max_std", ctypes.c_double),
    ]


class Proposals(ctypes.Structure):
    """bcmpc_proposals (40 bytes): given action sequences in every iteration's population (bc_mpc_amd/proposals.py);
    ``sequences`` is a host pointer (``device`` 0, canonical ``[n_envs][P][H][A]``) or a device pointer (``device``
    1, read through the three element strides)."""
    _fields_ = [
        ("sequences", ctypes.c_void_p),
        ("count", ctypes.c_int32),
        ("device", ctypes.c_int32),
        ("env_stride", ctypes.c_int64),
        ("seq_stride", ctypes.c_int64),
        ("step_stride", ctypes.c_int64),
    ]


class Knots(ctypes.Structure):
    """bcmpc_knots (8 bytes): ``count`` knots per action dimension interpolated to the horizon (bc_mpc_amd/knots.py);
    ``kind`` indexes ``knots.KINDS`` (hold, linear, cubic); count 0 is off."""
    _fields_ = [
        ("count", ctypes.c_int32),
        ("kind", ctypes.c_int32),
    ]


class MppiStats(ctypes.Structure):
    """One MPPI update's statistics (bcmpc_mppi_stats); no valid candidate: 0, 0, NaN, 0."""
    _fields_ = [
        ("weight_sum", ctypes.c_double),
        ("ess", ctypes.c_double),
        ("min_cost", ctypes.c_double),
        ("n_valid", ctypes.c_int64),
    ]


class Result(ctypes.Structure):
    _fields_ = [
        ("best_index", ctypes.c_int64),
        ("best_cost", ctypes.c_double),
        ("first_action", ctypes.c_double * MAX_ACTION),
    ]


# (name, restype, argtypes) -- every symbol include/bcmpc.h declares
class FitConfig(ctypes.Structure):
    _fields_ = [
        ("state_dim", ctypes.c_int32),
        ("action_dim", ctypes.c_int32),
        ("hidden", ctypes.c_int32),
        ("n_layers", ctypes.c_int32),
        ("activation", ctypes.c_int32),
        ("layer_norm", ctypes.c_int32),
        ("batch_size", ctypes.c_int32),
        ("device", ctypes.c_int32),
        ("learning_rate", ctypes.c_float),
        ("beta1", ctypes.c_float),
        ("beta2", ctypes.c_float),
        ("epsilon", ctypes.c_float),
        ("model", ctypes.c_int32),
    ]


class AcPpoConfig(ctypes.Structure):
    """bcmpc_acppo_config: the PPO optimizer's Adam constants (bc_mpc_amd/ppo.py)."""
    _fields_ = [
        ("beta1", ctypes.c_float),
        ("beta2", ctypes.c_float),
        ("epsilon", ctypes.c_float),
    ]


class AcFitConfig(ctypes.Structure):
    """bcmpc_acfit_config: one head of the actor-critic fitter (bc_mpc_amd/ac_fit.py)."""
    _fields_ = [
        ("state_dim", ctypes.c_int32),
        ("out_dim", ctypes.c_int32),
        ("hidden", ctypes.c_int32),
        ("n_layers", ctypes.c_int32),
        ("head", ctypes.c_int32),
        ("batch_size", ctypes.c_int32),
        ("device", ctypes.c_int32),
        ("beta1", ctypes.c_float),
        ("beta2", ctypes.c_float),
        ("epsilon", ctypes.c_float),
    ]


ACFIT_POLICY, ACFIT_VALUE = 0, 1

SIGNATURES = [
    ("bcmpc_abi_version", ctypes.c_int, []),
    ("bcmpc_last_error", ctypes.c_char_p, []),
    ("bcmpc_create", ctypes.c_int, [ctypes.POINTER(Config), ctypes.POINTER(ctypes.c_void_p)]),
    ("bcmpc_destroy", ctypes.c_int, [ctypes.c_void_p]),
    ("bcmpc_set_weights", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Weights), ctypes.c_uint64]),
    ("bcmpc_weights_version", ctypes.c_uint64, [ctypes.c_void_p]),
    ("bcmpc_predraw_stats", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    ("bcmpc_set_policy", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Policy), ctypes.c_uint64]),
    ("bcmpc_first_actions", ctypes.c_int, [ctypes.c_void_p, _DP]),
    ("bcmpc_set_discount", ctypes.c_int, [ctypes.c_void_p, ctypes.c_double]),
    ("bcmpc_set_action_bounds", ctypes.c_int, [ctypes.c_void_p, _DP, _DP]),
    ("bcmpc_set_cost_terms", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(CostTerm), ctypes.c_int32]),
    ("bcmpc_trajectory_cost_async", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int64, ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    ("bcmpc_terminal_value_supported", ctypes.c_int, [ctypes.POINTER(Config)]),
    ("bcmpc_set_terminal_value", ctypes.c_int,
     [ctypes.c_void_p, ctypes.POINTER(ValueNet), ctypes.c_double, ctypes.c_uint64]),
    ("bcmpc_terminal_value_async", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
      ctypes.c_void_p]),
    ("bcmpc_last_terminal_values", ctypes.c_int,
     [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_int32, _FP]),
    ("bcmpc_set_termination", ctypes.c_int,
     [ctypes.c_void_p, ctypes.POINTER(CostTerm), ctypes.c_int32, ctypes.c_double]),
    ("bcmpc_trajectory_cost_steps_async", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int64, ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("bcmpc_terminal_value_masked_async", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]),
    ("bcmpc_last_termination_steps", ctypes.c_int,
     [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]),
    ("bcmpc_set_cost_terms_x", ctypes.c_int,
     [ctypes.c_void_p, ctypes.POINTER(CostTermX), ctypes.c_int32, ctypes.c_int32]),
    ("bcmpc_set_cost_inputs", ctypes.c_int, [ctypes.c_void_p, _DP, ctypes.c_int32, ctypes.c_int32, _DP, ctypes.c_int32]),
    ("bcmpc_trajectory_cost_inputs_async", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int64, ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
      ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]),
    ("bcmpc_cost_input_buffers", ctypes.c_int,
     [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p)]),
    ("bcmpc_get_action", ctypes.c_int,
     [ctypes.c_void_p, _DP, _DP, ctypes.c_uint64, ctypes.c_int64, ctypes.POINTER(Result), _DP]),
    ("bcmpc_get_actions_batch", ctypes.c_int,
     [ctypes.c_void_p, _DP, ctypes.c_int32, _DP, ctypes.c_uint64, ctypes.c_int64, ctypes.POINTER(Result), _DP]),
    ("bcmpc_rollout_batch_async", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int64,
      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("bcmpc_get_action_mt19937", ctypes.c_int,
     [ctypes.c_void_p, _DP, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32), _DP, _DP,
      ctypes.c_int64, ctypes.c_int64, ctypes.c_uint64, ctypes.POINTER(Result), _DP]),
    ("bcmpc_mt19937_uniform", ctypes.c_int,
     [ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32), _DP, _DP, ctypes.c_int32, ctypes.c_int64,
      _DP]),
    ("bcmpc_mt19937_uniform_par", ctypes.c_int,
     [ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32), _DP, _DP, ctypes.c_int32, ctypes.c_int64,
      ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, _DP, ctypes.c_int32, ctypes.c_int64,
      ctypes.POINTER(ctypes.c_int32)]),
    ("bcmpc_rollout_async", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int64,
      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("bcmpc_rollout_policy_async", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int64, ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("bcmpc_cem_get_action", ctypes.c_int,
     [ctypes.c_void_p, _DP, ctypes.POINTER(Cem), ctypes.c_uint64, _DP, _DP, ctypes.POINTER(Result)]),
    ("bcmpc_cem_rollout_async", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int32,
      ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]),
    ("bcmpc_select_async", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32,
      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("bcmpc_cem_refit_async", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int32, ctypes.c_double,
      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("bcmpc_mppi_get_action", ctypes.c_int,
     [ctypes.c_void_p, _DP, ctypes.POINTER(Mppi), ctypes.c_uint64, _DP, _DP, ctypes.POINTER(Result),
      ctypes.POINTER(MppiStats)]),
    ("bcmpc_mppi_update_async", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int32,
      ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("bcmpc_cem_get_actions_batch", ctypes.c_int,
     [ctypes.c_void_p, _DP, ctypes.c_int32, ctypes.POINTER(Cem), ctypes.c_uint64, ctypes.c_int64, _DP, _DP,
      ctypes.POINTER(Result), _DP]),
    ("bcmpc_mppi_get_actions_batch", ctypes.c_int,
     [ctypes.c_void_p, _DP, ctypes.c_int32, ctypes.POINTER(Mppi), ctypes.c_uint64, ctypes.c_int64, _DP, _DP,
      ctypes.POINTER(Result), ctypes.POINTER(MppiStats), _DP]),
    ("bcmpc_plan_sample_async", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64,
      ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    ("bcmpc_plan_argmin_async", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32,
      ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]),
    ("bcmpc_select_batch_async", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32,
      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("bcmpc_cem_refit_batch_async", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64,
      ctypes.c_int32, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
      ctypes.c_int64, ctypes.c_void_p]),
    ("bcmpc_mppi_update_batch_async", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_uint64,
      ctypes.c_int32, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
      ctypes.c_void_p]),
    ("bcmpc_cem_get_action_s", ctypes.c_int,
     [ctypes.c_void_p, _DP, ctypes.POINTER(Cem), ctypes.POINTER(Sampling), ctypes.c_uint64, _DP, _DP,
      ctypes.POINTER(Result)]),
    ("bcmpc_mppi_get_action_s", ctypes.c_int,
     [ctypes.c_void_p, _DP, ctypes.POINTER(Mppi), ctypes.POINTER(Sampling), ctypes.c_uint64, _DP, _DP,
      ctypes.POINTER(Result), ctypes.POINTER(MppiStats)]),
    ("bcmpc_cem_get_actions_batch_s", ctypes.c_int,
     [ctypes.c_void_p, _DP, ctypes.c_int32, ctypes.POINTER(Cem), ctypes.POINTER(Sampling), ctypes.c_uint64,
      ctypes.c_int64, _DP, _DP, ctypes.POINTER(Result), _DP]),
    ("bcmpc_mppi_get_actions_batch_s", ctypes.c_int,
     [ctypes.c_void_p, _DP, ctypes.c_int32, ctypes.POINTER(Mppi), ctypes.POINTER(Sampling), ctypes.c_uint64,
      ctypes.c_int64, _DP, _DP, ctypes.POINTER(Result), ctypes.POINTER(MppiStats), _DP]),
    ("bcmpc_plan_sample_corr_async", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64,
      ctypes.c_int32, ctypes.c_int64, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
      ctypes.c_void_p, ctypes.c_void_p]),
    ("bcmpc_plan_keep_async", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64,
      ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("bcmpc_mppi_get_action_x", ctypes.c_int,
     [ctypes.c_void_p, _DP, ctypes.POINTER(Mppi), ctypes.POINTER(Sampling), ctypes.POINTER(MppiExt), ctypes.c_uint64,
      _DP, _DP, ctypes.POINTER(Result), ctypes.POINTER(MppiStats)]),
    ("bcmpc_mppi_get_actions_batch_x", ctypes.c_int,
     [ctypes.c_void_p, _DP, ctypes.c_int32, ctypes.POINTER(Mppi), ctypes.POINTER(Sampling), ctypes.POINTER(MppiExt),
      ctypes.c_uint64, ctypes.c_int64, _DP, _DP, ctypes.POINTER(Result), ctypes.POINTER(MppiStats), _DP]),
    ("bcmpc_mppi_control_cost_async", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]),
    ("bcmpc_mppi_sigma_update_async", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double,
      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_void_p]),
    ("bcmpc_cem_get_action_p", ctypes.c_int,
     [ctypes.c_void_p, _DP, ctypes.POINTER(Cem), ctypes.POINTER(Sampling), ctypes.POINTER(Proposals), ctypes.c_uint64,
      _DP, _DP, ctypes.POINTER(Result)]),
    ("bcmpc_mppi_get_action_p", ctypes.c_int,
     [ctypes.c_void_p, _DP, ctypes.POINTER(Mppi), ctypes.POINTER(Sampling), ctypes.POINTER(MppiExt),
      ctypes.POINTER(Proposals), ctypes.c_uint64, _DP, _DP, ctypes.POINTER(Result), ctypes.POINTER(MppiStats)]),
    ("bcmpc_cem_get_actions_batch_p", ctypes.c_int,
     [ctypes.c_void_p, _DP, ctypes.c_int32, ctypes.POINTER(Cem), ctypes.POINTER(Sampling), ctypes.POINTER(Proposals),
      ctypes.c_uint64, ctypes.c_int64, _DP, _DP, ctypes.POINTER(Result), _DP]),
    ("bcmpc_mppi_get_actions_batch_p", ctypes.c_int,
     [ctypes.c_void_p, _DP, ctypes.c_int32, ctypes.POINTER(Mppi), ctypes.POINTER(Sampling), ctypes.POINTER(MppiExt),
      ctypes.POINTER(Proposals), ctypes.c_uint64, ctypes.c_int64, _DP, _DP, ctypes.POINTER(Result),
      ctypes.POINTER(MppiStats), _DP]),
    ("bcmpc_plan_sample_prop_async", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64,
      ctypes.c_int32, ctypes.c_int64, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
      ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
      ctypes.c_void_p]),
    ("bcmpc_rollout_policy_batch_async", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int64,
      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("bcmpc_cem_get_action_k", ctypes.c_int,
     [ctypes.c_void_p, _DP, ctypes.POINTER(Cem), ctypes.POINTER(Sampling), ctypes.POINTER(Proposals),
      ctypes.POINTER(Knots), ctypes.c_uint64, _DP, _DP, ctypes.POINTER(Result)]),
    ("bcmpc_mppi_get_action_k", ctypes.c_int,
     [ctypes.c_void_p, _DP, ctypes.POINTER(Mppi), ctypes.POINTER(Sampling), ctypes.POINTER(MppiExt),
      ctypes.POINTER(Proposals), ctypes.POINTER(Knots), ctypes.c_uint64, _DP, _DP, ctypes.POINTER(Result),
      ctypes.POINTER(MppiStats)]),
    ("bcmpc_cem_get_actions_batch_k", ctypes.c_int,
     [ctypes.c_void_p, _DP, ctypes.c_int32, ctypes.POINTER(Cem), ctypes.POINTER(Sampling), ctypes.POINTER(Proposals),
      ctypes.POINTER(Knots), ctypes.c_uint64, ctypes.c_int64, _DP, _DP, ctypes.POINTER(Result), _DP]),
    ("bcmpc_mppi_get_actions_batch_k", ctypes.c_int,
     [ctypes.c_void_p, _DP, ctypes.c_int32, ctypes.POINTER(Mppi), ctypes.POINTER(Sampling), ctypes.POINTER(MppiExt),
      ctypes.POINTER(Proposals), ctypes.POINTER(Knots), ctypes.c_uint64, ctypes.c_int64, _DP, _DP,
      ctypes.POINTER(Result), ctypes.POINTER(MppiStats), _DP]),
    ("bcmpc_plan_sample_knots_async", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64,
      ctypes.c_int32, ctypes.c_int64, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
      ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("bcmpc_cem_refit_batch_steps_async", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64,
      ctypes.c_int32, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
      ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p]),
    ("bcmpc_mppi_update_batch_steps_async", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_uint64,
      ctypes.c_int32, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
      ctypes.c_int32, ctypes.c_void_p]),
    ("bcmpc_plan_keep_steps_async", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64,
      ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]),
    ("bcmpc_mppi_control_cost_steps_async", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]),
    ("bcmpc_mppi_sigma_update_steps_async", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double,
      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int32,
      ctypes.c_void_p]),
    ("bcmpc_ensemble_create", ctypes.c_int, [ctypes.POINTER(Config), ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p)]),
    ("bcmpc_ensemble_destroy", ctypes.c_int, [ctypes.c_void_p]),
    ("bcmpc_ensemble_size", ctypes.c_int, [ctypes.c_void_p]),
    ("bcmpc_ensemble_member", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p)]),
    ("bcmpc_ensemble_set_rule", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_double]),
    ("bcmpc_ensemble_get_action", ctypes.c_int,
     [ctypes.c_void_p, _DP, _DP, ctypes.c_uint64, ctypes.c_int64, ctypes.POINTER(Result), _DP, _DP]),
    ("bcmpc_ensemble_get_actions_batch", ctypes.c_int,
     [ctypes.c_void_p, _DP, ctypes.c_int32, _DP, ctypes.c_uint64, ctypes.c_int64, ctypes.POINTER(Result), _DP,
      _DP]),
    ("bcmpc_ensemble_cem_get_action", ctypes.c_int,
     [ctypes.c_void_p, _DP, ctypes.POINTER(Cem), ctypes.c_uint64, _DP, _DP, ctypes.POINTER(Result)]),
    ("bcmpc_ensemble_mppi_get_action", ctypes.c_int,
     [ctypes.c_void_p, _DP, ctypes.POINTER(Mppi), ctypes.c_uint64, _DP, _DP, ctypes.POINTER(Result),
      ctypes.POINTER(MppiStats)]),
    ("bcmpc_ensemble_reduce_async", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32,
      ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]),
    ("bcmpc_stream", ctypes.c_void_p, [ctypes.c_void_p]),
    ("bcmpc_engine_status", ctypes.c_int, [ctypes.c_void_p]),
    ("bcmpc_engine_team_reruns", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    ("bcmpc_select_results_async", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]),
    ("bcmpc_engine_set_timing", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32]),
    ("bcmpc_last_kernel_ms", ctypes.c_int,
     [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]),
    ("bcmpc_fit_create", ctypes.c_int, [ctypes.POINTER(FitConfig), ctypes.POINTER(ctypes.c_void_p)]),
    ("bcmpc_fit_destroy", ctypes.c_int, [ctypes.c_void_p]),
    ("bcmpc_fit_is_fused", ctypes.c_int, [ctypes.c_void_p]),
    ("bcmpc_fit_set_params", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Weights)]),
    ("bcmpc_fit_get_params", ctypes.c_int,
     [ctypes.c_void_p, ctypes.POINTER(_FP), ctypes.POINTER(_FP), ctypes.POINTER(_FP), ctypes.POINTER(_FP)]),
    ("bcmpc_fit_set_data", ctypes.c_int, [ctypes.c_void_p, _DP, _DP, _DP, ctypes.c_int64]),
    ("bcmpc_fit_run", ctypes.c_int,
     [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, _FP]),
    ("bcmpc_fit_last_error", ctypes.c_char_p, []),
    ("bcmpc_fit_set_rewards", ctypes.c_int, [ctypes.c_void_p, _DP, ctypes.c_int64]),
    ("bcmpc_fit_reward_losses", ctypes.c_int, [ctypes.c_void_p, _FP]),
    ("bcmpc_acfit_create", ctypes.c_int, [ctypes.POINTER(AcFitConfig), ctypes.POINTER(ctypes.c_void_p)]),
    ("bcmpc_acfit_destroy", ctypes.c_int, [ctypes.c_void_p]),
    ("bcmpc_acfit_set_params", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(_FP), ctypes.POINTER(_FP)]),
    ("bcmpc_acfit_get_params", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(_FP), ctypes.POINTER(_FP)]),
    ("bcmpc_acfit_set_filter", ctypes.c_int, [ctypes.c_void_p, _FP, _FP]),
    ("bcmpc_acfit_set_data", ctypes.c_int, [ctypes.c_void_p, _DP, _DP, ctypes.c_int64]),
    ("bcmpc_acfit_run", ctypes.c_int,
     [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32), ctypes.c_int32,
      ctypes.c_float, _FP]),
    ("bcmpc_acfit_is_graph", ctypes.c_int, [ctypes.c_void_p]),
    ("bcmpc_acfit_lds_words", ctypes.c_int64,
     [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]),
    ("bcmpc_acfit_last_error", ctypes.c_char_p, []),
    ("bcmpc_acppo_create", ctypes.c_int,
     [ctypes.POINTER(AcPpoConfig), ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]),
    ("bcmpc_acppo_destroy", ctypes.c_int, [ctypes.c_void_p]),
    ("bcmpc_acppo_set_logstd", ctypes.c_int, [ctypes.c_void_p, _FP]),
    ("bcmpc_acppo_get_logstd", ctypes.c_int, [ctypes.c_void_p, _FP]),
    ("bcmpc_acppo_set_old", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(_FP), ctypes.POINTER(_FP), _FP, _FP, _FP]),
    ("bcmpc_acppo_set_data", ctypes.c_int, [ctypes.c_void_p, _DP, _FP, _FP, _FP, ctypes.c_int64]),
    ("bcmpc_acppo_run", ctypes.c_int,
     [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.c_float,
      ctypes.c_float, ctypes.c_float, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32), ctypes.c_float,
      _FP, _FP]),
    ("bcmpc_acppo_is_graph", ctypes.c_int, [ctypes.c_void_p]),
    ("bcmpc_acppo_check_pair", ctypes.c_int,
     [ctypes.POINTER(AcPpoConfig), ctypes.POINTER(AcFitConfig), ctypes.POINTER(AcFitConfig)]),
    ("bcmpc_acppo_check_run", ctypes.c_int,
     [ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.c_int64, ctypes.c_float,
      ctypes.c_float, ctypes.c_float]),
    ("bcmpc_acppo_lds_words", ctypes.c_int64, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]),
    ("bcmpc_acppo_last_error", ctypes.c_char_p, []),
    ("bcmpc_comm_unique_id", ctypes.c_int, [ctypes.POINTER(ctypes.c_uint8)]),
    ("bcmpc_comm_init", ctypes.c_int,
     [ctypes.POINTER(ctypes.c_uint8), ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p)]),
    ("bcmpc_comm_destroy", ctypes.c_int, [ctypes.c_void_p]),
    ("bcmpc_engine_set_comm", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    ("bcmpc_select_results", ctypes.c_int, [ctypes.POINTER(Result), ctypes.c_int32, ctypes.c_int32,
                                            ctypes.POINTER(Result)]),
    ("bcmpc_mt19937_uniform_device", ctypes.c_int,
     [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32), _DP, _DP, ctypes.c_int64,
      ctypes.c_int64, _DP]),
    ("bcmpc_engine_layout", ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int32]),
    ("bcmpc_split_pp_lds_bytes", ctypes.c_int64, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]),
    ("bcmpc_engine_info", ctypes.c_int,
     [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64),
      ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
]

_lib = None


def load() -> ctypes.CDLL:
    """Load libbcmpc.so once; raise ImportError (loudly) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"libbcmpc.so not found at {LIB_PATH}: build it with `make` or "
            "`python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback exists)")
    lib = ctypes.CDLL(LIB_PATH)
    for name, res, args in SIGNATURES:
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.bcmpc_abi_version() != ABI_VERSION:
        raise ImportError(f"libbcmpc ABI {lib.bcmpc_abi_version()} != expected {ABI_VERSION}")
    _lib = lib
    return lib


class BcmpcError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"[bcmpc status {code}] {msg}")
        self.code = code


def check(code: int, fit: bool = False) -> None:
    if code == OK:
        return
    lib = load()
    msg = (lib.bcmpc_fit_last_error() if fit else lib.bcmpc_last_error()).decode(errors="replace")
    if code == ERR_EMPTY:
        raise ValueError(msg)                  # np.argmin on an empty sequence
    if code in (ERR_ARG, ERR_UNSUPPORTED):
        raise ValueError(f"[bcmpc status {code}] {msg}")
    raise BcmpcError(code, msg)
