"""MI355X-native Real-ESRGAN (RRDBNet) inference path for NESR.

Drop-in objects for the two third-party classes the reference constructs
(nesr/nesr.py:161-162,216-229; standalone/direct_esrgan.py:92-93,104,118-127):

    from neural_enhanced_super_resolution_amd import RRDBNet, RealESRGANer

or, with ``<repo>/dropin`` on PYTHONPATH, the reference's own import lines
(``from basicsr.archs.rrdbnet_arch import RRDBNet``; ``from realesrgan import RealESRGANer``)
resolve to these classes unchanged.  The network forward runs in hand-written HIP kernels
(libnesr_hip.so, C ABI in include/nesr_hip.h); there is no CPU fallback.
"""
from .rrdbnet import RRDBNet, conv3x3, last_conv_kernel, rrdbnet_state_dict_spec  # noqa: F401
from .srvgg import SRVGGNetCompact, srvgg_state_dict_spec  # noqa: F401
from .realesrganer import RealESRGANer  # noqa: F401
from .segformer import SegFormer, segformer_state_dict_spec  # noqa: F401
from .swin2sr import Swin2SR, swin2sr_state_dict_spec  # noqa: F401
from .vae import VaeDecoder, vae_state_dict_spec  # noqa: F401
from .unet import UNet2DCondition, unet_state_dict_spec  # noqa: F401
from .clip_text import ClipTextEncoder, clip_text_state_dict_spec  # noqa: F401
from .sdx4 import StableDiffusionX4Upscaler  # noqa: F401

__all__ = ["ClipTextEncoder", "RRDBNet", "RealESRGANer", "SRVGGNetCompact", "SegFormer", "StableDiffusionX4Upscaler", "Swin2SR", "UNet2DCondition", "VaeDecoder", "clip_text_state_dict_spec", "conv3x3", "rrdbnet_state_dict_spec", "segformer_state_dict_spec",
           "srvgg_state_dict_spec", "swin2sr_state_dict_spec", "unet_state_dict_spec", "vae_state_dict_spec"]
__version__ = "0.1.0"
