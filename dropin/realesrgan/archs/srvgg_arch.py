"""Shim: ``from realesrgan.archs.srvgg_arch import SRVGGNetCompact`` (upstream's realesr-general-x4v3 /
realesr-animevideov3 network) resolves to the MI355X-native class."""
from neural_enhanced_super_resolution_amd.srvgg import SRVGGNetCompact  # noqa: F401
