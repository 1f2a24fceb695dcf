"""MI355X-native encode -> quantize -> synthesize path of yubster4525/image_compression_2.

Drop-in classes (same names / signatures as the reference modules):
  stylegan3_hvae_full:        HVAE_VGG_Encoder, VGGBlock, HierarchyProjector, StyleGAN3Compressor,
                              save_tensor_as_image
  gumbel_softmax_compression: GumbelSoftmaxDiscretization, GumbelSoftmaxCompressor
  networks_stylegan3:         Generator (G_ema duck type; T, and R with SG3_R_KWARGS), SynthesisNetwork, ...
  sg3_ops:                    bias_act, upfirdn2d, filtered_lrelu  (torch_utils.ops mirrors)
  cabac_compression:          ContextModel, cabac_encode / cabac_decode, CABACCompressor (native range coder)
  legacy:                     load_network_pkl (SG3 pickle loader that executes nothing from the file)
  metrics:                    uint8_quality, ssim, evaluate_compression (the PSNR + SSIM record of test_compression);
                              ms_ssim_terms, uint8_ms_ssim, ms_ssim (the MS-SSIM figure), ms_ssim_loss, MSSSIMLoss
                              (1 - MS-SSIM with a HIP backward: the perceptual training term that works offline)
  image_io:                   resize_u8 / to_tensor (Pillow's 8-bit Resize + ToTensor + Normalize, bit for bit, on
                              ragged uint8 batches), to_uint8 / save_images (the three f32 -> uint8 conversions),
                              ImageDataset, image_batches (the reference's dataset with the transform on the device)
All compute runs in libic2ops.so (hand-written HIP for gfx950); ROCm tensors only.
"""
from . import _native  # noqa: F401
from .stylegan3_hvae_full import (HVAE_VGG_Encoder, VGGBlock, HierarchyProjector, StyleGAN3Compressor,  # noqa: F401
                                  save_tensor_as_image, quantize_uniform, resize_bilinear)
from .gumbel_softmax_compression import GumbelSoftmaxDiscretization, GumbelSoftmaxCompressor  # noqa: F401
from .networks_stylegan3 import (Generator, SynthesisNetwork, SynthesisLayer, SynthesisInput,  # noqa: F401
                                 MappingNetwork, FullyConnectedLayer, make_generator, SG3_R_KWARGS)
from . import sg3_ops  # noqa: F401
from .cabac_compression import CABACCompressor, ContextModel, cabac_encode, cabac_decode  # noqa: F401
from . import legacy  # noqa: F401
from .metrics import uint8_quality, ssim, ssim_from_sums, evaluate_compression  # noqa: F401
from .metrics import ms_ssim_terms, uint8_ms_ssim, ms_ssim, ms_ssim_loss, MSSSIMLoss, MS_SSIM_TILE  # noqa: F401
from . import image_io  # noqa: F401
from .image_io import (resample_tables, resize_u8, to_tensor, to_uint8, save_images, ImageDataset,  # noqa: F401
                       image_batches)

__all__ = ["HVAE_VGG_Encoder", "VGGBlock", "HierarchyProjector", "StyleGAN3Compressor", "save_tensor_as_image",
           "GumbelSoftmaxDiscretization", "GumbelSoftmaxCompressor", "Generator", "SynthesisNetwork",
           "SynthesisLayer", "SynthesisInput", "MappingNetwork", "FullyConnectedLayer", "make_generator", "SG3_R_KWARGS",
           "quantize_uniform", "resize_bilinear", "sg3_ops", "CABACCompressor", "ContextModel", "cabac_encode",
           "cabac_decode", "legacy", "uint8_quality", "ssim", "ssim_from_sums", "evaluate_compression",
           "ms_ssim_terms", "uint8_ms_ssim", "ms_ssim", "ms_ssim_loss", "MSSSIMLoss", "MS_SSIM_TILE",
           "image_io", "resample_tables", "resize_u8", "to_tensor", "to_uint8", "save_images", "ImageDataset",
           "image_batches"]
