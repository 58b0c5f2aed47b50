"""atc_hip — host side of the MI355X-native batched AtcGym.step() path (device state in PyTorch-ROCm tensors, kernels
in libatcstep.so reached through ctypes)."""
from . import layout  # noqa: F401
from . import evaluate  # noqa: F401  (summary / evaluate: torch is imported where they run)
