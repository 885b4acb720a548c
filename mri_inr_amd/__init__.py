"""mri_inr_amd -- MI355X-native modulated-SIREN inference path (drop-in for one path of mri-inr).

Public surface mirrors the reference's: ``ModulatedSiren`` (src/networks/modulated_siren.py) and
``load_configuration`` (src/configuration/configuration.py).  Compute lives in libmsiren.so
(hand-written gfx950 HIP kernels behind the C ABI of include/msiren.h).
"""

from .configuration import load_configuration, model_kwargs  # noqa: F401
from .model import ModulatedSiren  # noqa: F401
from .volume import plane_points  # noqa: F401
from . import align  # noqa: F401  (map helpers, and the step rule of ModulatedSiren.align_solve: lm_step, solve_on_host)
from . import align_volume  # noqa: F401  (the same for ModulatedSiren.align_volume_cost / align_volume_solve: 3 x 3 maps, lm_step_v)

__all__ = ["ModulatedSiren", "load_configuration", "model_kwargs", "plane_points", "align", "align_volume"]
__version__ = "0.1.0"
