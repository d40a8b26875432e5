"""grl_amd -- MI355X-native runner for grl's OnlineLearningExperiment hot path.

The product is the HIP library behind include/grlx.h (grl_amd/csrc); this
package is its ctypes host.  Importing does not load the library; the first use
does, and fails loudly when it has not been built (no CPU fallback).
"""
from . import capi, runner  # noqa: F401
from .runner import EnsembleEvaluation, EnsembleResult, EnsembleTrajectory, Evaluation, Trajectory, FqiRunner, Runner, observation_grid, acrobot_q_config, pendulum_fqi_config, cart_pole_ac_config, compass_walker_q_config, pendulum_sarsa_config, snapshot_info, sweep_grid  # noqa: F401
from .runner import SampledEvaluation, SampledTrajectory, episode_streams  # noqa: F401
from .runner import NoisyEvaluation, NoisyTrajectory, episode_stream_words  # noqa: F401
from .runner import ActorEnsembleEvaluation, ActorEnsembleTrajectory  # noqa: F401

__all__ = ["capi", "runner", "Runner", "FqiRunner", "pendulum_fqi_config", "pendulum_sarsa_config", "cart_pole_ac_config", "acrobot_q_config", "compass_walker_q_config", "sweep_grid", "snapshot_info", "observation_grid", "EnsembleResult", "Evaluation", "EnsembleEvaluation", "Trajectory", "EnsembleTrajectory",
           "SampledEvaluation", "SampledTrajectory", "episode_streams", "NoisyEvaluation", "NoisyTrajectory", "episode_stream_words",
           "ActorEnsembleEvaluation", "ActorEnsembleTrajectory"]
