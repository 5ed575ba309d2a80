"""cooperative-search_amd: MI355X-native batched flight_easy / flight environment path.

Scope: the environment reset/step/reward/obs/state path of
WZN1ng/Cooperative-Search, advanced by hand-written gfx950 HIP kernels behind the C ABI of
include/coopsearch.h.  Nothing here falls back to a CPU implementation: importing works anywhere, but
constructing an environment without the built HIP library and a GPU raises.
"""
from .targets import load_targets, DEFAULT_TARGETS_FILE, default_circle_dict  # noqa: F401
from .args import get_flight_easy_args, get_flight_args, make_env_args, apply_env_info  # noqa: F401
from .env import BatchedFlightEnv, FlightSearchEnvEasy, FlightSearchEnv  # noqa: F401
from . import _lib as lib  # noqa: F401
from . import dist  # noqa: F401
from .replay import COMPACT_KEYS, CompactReplayBuffer, DeviceReplayBuffer, compact_from_dense, expand_compact  # noqa: F401
from .agents import AgentRNN, BatchedAgents, FusedAgents, rnn_input_shape  # noqa: F401
from .collector import EpisodeCollector, EpsilonSchedule, evaluate, collect_experiment_data, random_policy  # noqa: F401
from .learner import GRUSequence, MixerNet, QMixLearner, get_mixer_args, unroll_q  # noqa: F401
from .learner import DOPLearner, OffPGCritic, ReinforceLearner, get_dop_args, get_reinforce_args  # noqa: F401
from .learner import PPOLearner, PPOPolicyLoss, ValueCritic, gae, get_ppo_args  # noqa: F401
from .runner import Runner, get_model_idx, run_name  # noqa: F401
from .snapshot import EnvSnapshot  # noqa: F401
from .baseline import CoverageAgents, coverage_actions_torch  # noqa: F401
from .local import LocalCoverageAgents, local_coverage_actions_torch  # noqa: F401
from .sweep import SweepResult, sweep_episodes, sweep_episodes_torch, sweep_batch, swept_curve, sweep_efficiency  # noqa: F401
from .sweep import sweep_bonus, with_sweep_bonus, collect_sweep_data  # noqa: F401
from .motion import TargetMotion, MovingTargetEnv, move_targets_torch, make_env  # noqa: F401
from .belief import BeliefAgents, BeliefModel, belief_actions_torch  # noqa: F401
from .local_belief import LocalBeliefAgents, local_belief_actions_torch  # noqa: F401
from .plan import PlanAgents, plan_actions_torch  # noqa: F401
from .local_plan import LocalPlanAgents, local_plan_actions_torch  # noqa: F401
from .forecast import ForecastAgents, forecast_torch, plan_forecast_actions_torch  # noqa: F401
from .local_forecast import LocalForecastAgents, local_forecast_torch, local_plan_forecast_actions_torch  # noqa: F401
from .imitate import BCLoss, ExpertParams, ImitationLearner, LabelledRing, bc_loss_torch, distil, expert_params, get_bc_args  # noqa: F401
from .imitate import label_episodes, label_episodes_hip, label_episodes_torch  # noqa: F401
from .gridobs import FeatureRing, GridAgents, GridImitationLearner, distil_grid, feature_episodes, feature_episodes_hip  # noqa: F401
from .gridobs import feature_episodes_torch, grid_features, grid_features_hip, grid_features_torch  # noqa: F401
from .localobs import LocalExpertParams, LocalGridAgents, distil_local_grid, local_expert_params, local_feature_episodes  # noqa: F401
from .localobs import local_feature_episodes_hip, local_feature_episodes_torch, local_grid_features, local_grid_features_hip  # noqa: F401
from .localobs import local_grid_features_torch, local_label_episodes  # noqa: F401
from .render import RenderSpec, episode_tables, render_episodes, render_episodes_torch, write_frames  # noqa: F401

__all__ = ["BatchedFlightEnv", "FlightSearchEnvEasy", "FlightSearchEnv", "load_targets", "default_circle_dict",
           "get_flight_easy_args", "get_flight_args", "make_env_args", "lib"]
