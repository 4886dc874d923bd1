"""stereo-3d-reconstruction_amd — MI355X (gfx950) forward path of a Stereo2Voxel / Stereo2Point network.

Scope: the data-parallel hot path only: stereo feature encoder, disparity cost
volume, 3D-conv voxel decoder, point head + Chamfer distance, behind the `encoder` / `cost_volume`
/ `decoder` nn.Module API.  The network architecture is BUILD-SPECIFIED (arch_spec.py) because the
reference's model code is not in the mount (/root/reference/README.md:5).

Importing this package never touches the GPU and never loads the oracle; the HIP library
(csrc/libs3r_hip.so) is loaded on first use and its absence is a hard error.
"""
from . import arch_spec, checkpoint, collate, data, evaluate, exr
from .augment import AugmentConfig, StereoAugment, augment_pair
from .graph import GraphedForward, PrefetchingLoader
from ._lib import ALGO_AUTO, ALGO_DIRECT, ALGO_WINOGRAD, S3RError, LIB_PATH, load as load_library, profile_enable, profile_read, profile_reset, profile_detail
from .init import seed_module, seeded_state_dict, synthetic_pairs
from .modules import (CostVolume, Decoder, Encoder, PointHead, Stereo2Point, Stereo2Voxel, VolumeEncoder, cost_volume, debug_overrides,
                      decoder, DISPARITY_TEMPERATURE, encoder)
from .ops import (ChamferDistance, chamfer_distance, chamfer_distance_backward, differentiable_chamfer_distance, linear, linear_backward, differentiable_linear, VoxelBCELoss, voxel_bce, voxel_bce_backward, differentiable_voxel_bce, head, head_backward, differentiable_head, conv_forward, conv_backward, differentiable_conv, stem_backward, batchnorm_train_forward, batchnorm_train_backward, differentiable_batchnorm, cost_volume_backward, differentiable_cost_volume, disparity_epe, disparity_wta,
                  disparity_soft, disparity_metrics, voxel_iou,
                  disparity_soft_backward, differentiable_disparity_soft, DisparityLoss, disparity_loss, disparity_loss_backward,
                  differentiable_disparity_loss, SurfacePoints, voxel_surface_points)
from .optim import SGD, Adam, AdamW
from . import train
from .train import TrainConfig, fit

__all__ = [
    "GraphedForward", "PrefetchingLoader", "arch_spec", "checkpoint", "collate", "data", "evaluate", "S3RError", "LIB_PATH", "load_library", "profile_enable", "profile_read", "profile_reset", "profile_detail",
    "seed_module", "seeded_state_dict", "synthetic_pairs",
    "Encoder", "CostVolume", "Decoder", "VolumeEncoder", "PointHead", "Stereo2Voxel", "Stereo2Point",
    "ChamferDistance", "chamfer_distance", "chamfer_distance_backward", "differentiable_chamfer_distance", "linear", "linear_backward", "differentiable_linear", "VoxelBCELoss", "voxel_bce", "voxel_bce_backward", "differentiable_voxel_bce", "head", "head_backward", "differentiable_head", "conv_forward", "conv_backward", "differentiable_conv", "stem_backward", "batchnorm_train_forward", "batchnorm_train_backward", "differentiable_batchnorm", "cost_volume_backward", "differentiable_cost_volume", "debug_overrides", "ALGO_AUTO", "ALGO_DIRECT", "ALGO_WINOGRAD", "voxel_iou", "disparity_wta", "disparity_epe", "disparity_soft", "disparity_metrics", "DISPARITY_TEMPERATURE", "disparity_soft_backward", "differentiable_disparity_soft", "DisparityLoss", "disparity_loss", "disparity_loss_backward", "differentiable_disparity_loss", "SGD", "Adam", "AdamW", "AugmentConfig", "StereoAugment", "augment_pair", "SurfacePoints", "voxel_surface_points", "train", "TrainConfig", "fit", "encoder", "cost_volume", "decoder",
]
