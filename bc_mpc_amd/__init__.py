"""bc_mpc_amd -- MI355X-native random-shooting MPC rollout engine.

Drop-in for Bonnieccc/bc-mpc's ``controllers.MPCcontroller.get_action`` hot
path (controllers.py:57-88 -> dynamics.py:106-119 -> cost_functions.py:9-63),
and its siblings MPCcontrollerPolicyNet / MPCcontrollerReward /
MPCcontrollerPolicyNetReward / MCTScontrollerPolicyNetReward (controllers.py:90-457).
The compute path is libbcmpc.so (HIP, gfx950); see DESIGN.md.
"""
from . import _lib
from .controllers import (Controller, MCTScontrollerPolicyNetReward, MPCcontroller, MPCcontrollerPolicyNet,
                          MPCcontrollerPolicyNetReward, MPCcontrollerReward, RandomController)
from .cem import CEMcontroller
from .mppi import MPPIcontroller
from .cost_functions import TermCost, cheetah_cost_fn, cheetah_terms, trajectory_cost_fn
from .engine import BatchResult, MLPSpec, PolicySpec, RolloutEngine, StepResult
from .ensemble import EnsembleDynamicsModel, EnsembleEngine
from . import value
from .value import ValueSpec
from . import ac_fit
from . import ppo
from .ppo import gae, standardize
from .actor_critic import MlpActorCritic

__all__ = ["Controller", "MPCcontroller", "MPCcontrollerPolicyNet", "MPCcontrollerReward",
           "MPCcontrollerPolicyNetReward", "MCTScontrollerPolicyNetReward", "CEMcontroller", "MPPIcontroller", "RandomController", "PolicySpec", "cheetah_cost_fn",
           "trajectory_cost_fn", "TermCost", "cheetah_terms", "MLPSpec", "RolloutEngine", "StepResult", "BatchResult",
           "EnsembleEngine", "EnsembleDynamicsModel", "ValueSpec", "MlpActorCritic", "gae", "standardize"]

_lib.load()   # fail loudly at import when the HIP library is missing
