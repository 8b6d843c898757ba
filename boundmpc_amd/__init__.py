"""boundmpc_amd -- MI355X-native batched solver for the per-step optimal-control problem of
BoundMPC (Thieso/BoundMPC), behind the reference's own `solver(...)` / `BoundMPC.step()` API.

Only the hot path is here: HIP kernels + C ABI under csrc/, and the host
mirror of the reference interface.  No CPU fallback exists: without the HIP extension and a
GPU the solver constructors raise."""
from .solver import BatchedOCPSolver, NlpSolverShim  # noqa: F401
from ._lib import BoundMPCHipError, LIB_PATH  # noqa: F401

__all__ = ["BatchedOCPSolver", "NlpSolverShim", "BoundMPCHipError", "LIB_PATH"]

# the plant, sensor and observer models of a rollout (boundmpc_amd.stream), re-exported on first use: importing the package does not import the stream module
_PLANT = ("PLANT", "PLANT_STATE", "PLANT_REC", "plant_table", "plant_check", "plant_state_of", "plant_robot", "unpack_plant_rec",
          "SENSOR", "SENSOR_STATE", "SENSOR_REC", "sensor_table", "sensor_check", "sense_robot", "truth_robot", "unpack_sensor_rec",
          "OBSERVER", "OBSERVER_STATE", "OBSERVER_REC", "observer_table", "observer_check", "observe_robot", "unpack_observer_rec")


def __getattr__(name):
    if name in _PLANT:
        from . import stream
        return getattr(stream, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
