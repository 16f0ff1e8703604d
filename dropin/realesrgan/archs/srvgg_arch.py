"""Shim: ``from realesrgan.archs.srvgg_arch import SRVGGNetCompact`` (upstream's realesr-general-x4v3 /
realesr-animevideov3 network) resolves to the MI355X-native class.  Upstream's constructor has no compute_dtype: a model made
through this import runs the f32 form, or bf16 after ``.half()``; the fp16 form is ``SRVGGNetCompact(..., compute_dtype="fp16")``."""
from neural_enhanced_super_resolution_amd.srvgg import SRVGGNetCompact  # noqa: F401
