"""gptq_svd_amd -- MI355X-native TruncGPTQ per-layer solver (HIP kernels behind a C ABI).

The reference-compatible API lives in ``gptq_svd_amd.gptq_utils``.
"""
from . import _lib  # noqa: F401  (fails loudly if libtruncgptq.so is missing)
from . import export, harness, qlinear  # noqa: F401
from .export import load_quantized  # noqa: F401
from .gptq_utils import (HessianAccumulator, Quantizer, Sketcher, gptq_fwrd,  # noqa
                         log_quantization_error, next_power_of_2, pack_quantized,
                         process_hessian, process_hessian_alt, process_sketch,
                         triton_process_block, truncated_spectral_factor)
from .qlinear import (MXQuantLinear, QuantLinear, dequantize_packed,  # noqa: F401
                      dequantize_packed_mx)

__version__ = "0.1.0"
