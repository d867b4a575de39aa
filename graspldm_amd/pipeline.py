"""Convenience constructors for the shipped `fpc` experiment with synthetic weights
(no checkpoints exist offline)."""
import torch

from .builder import build_model_from_cfg
from .synthetic import load_synthetic_weights


def fpc_model_config(n_points=1024, scheduler="ddim", latent=4, pc_latent=64, pc_channels=3, encoder="PVCNNEncoder",
                     encoder_scale=None, use_global_attention=False, use_local_attention=False, vae_core="ResNet1D"):
    """configs/generation/fpc/fpc_1a_latentc3_z4_pc64_180k.py:25-153 as data.  encoder="PVCNN2Encoder": the same
    experiment conditioned by the SET-ABSTRACTION encoder family of the registry (pc_encoders.py:139-197 in its repaired
    form: PointNet++ set abstraction + PVConv + feature propagation, then the same head); encoder_scale =
    (scale_channels, scale_voxel_resolution), default the shipped (0.75, 0.75) / PVCNN2's own width (1, 1).
    use_global_attention: the encoder's attention block over all points (pc_encoders.py:65-69), off in the shipped config.
    use_local_attention (PVCNN2Encoder only): voxel attention inside the PVConv of the second set-abstraction stage
    (pc_encoders.py:152-153, ext/pvcnn/utils.py:123); the key is absent from the config when the flag is off.
    vae_core="Unet1D": the pose decoder and the grasp encoder on the registry's other 1-D core (grasp_vae.py:356,440), with
    dim_mults (1, 2, 4, 8) and no time conditioning; the denoiser is unchanged."""
    if vae_core not in ("ResNet1D", "Unet1D"):
        raise ValueError(f"vae_core must be ResNet1D or Unet1D, not {vae_core!r}")
    rn = dict(block_channels=(32, 64, 128, 256), input_conditioning_dims=pc_latent, resnet_block_groups=4, dropout=0.1)
    if use_local_attention and encoder != "PVCNN2Encoder":
        raise ValueError("use_local_attention is an argument of PVCNN2Encoder only")
    if encoder == "PVCNNEncoder":
        sc, sv = encoder_scale or (0.75, 0.75)
        enc = dict(type="PVCNNEncoder", args=dict(
            in_features=3, n_points=n_points, scale_channels=sc, scale_voxel_resolution=sv,
            num_blocks=(1, 1, 1, 1), out_channels=pc_channels, use_global_attention=bool(use_global_attention)))
    elif encoder == "PVCNN2Encoder":
        sc, sv = encoder_scale or (1, 1)
        enc = dict(type="PVCNN2Encoder", args=dict(
            in_features=3, n_points=n_points, scale_channels=sc, scale_voxel_resolution=sv, out_channels=pc_channels,
            **(dict(use_global_attention=True) if use_global_attention else {}),
            **(dict(use_local_attention=True) if use_local_attention else {})))
    else:
        raise ValueError(f"encoder must be PVCNNEncoder or PVCNN2Encoder, not {encoder!r}")
    core = rn if vae_core == "ResNet1D" else dict(dim_mults=(1, 2, 4, 8), input_conditioning_dims=pc_latent,
                                                  is_time_conditioned=False, resnet_block_groups=4)
    vae = dict(model=dict(type="GraspCVAE", args=dict(
        grasp_latent_size=latent, pc_latent_size=pc_latent,
        pc_encoder_config=enc,
        grasp_encoder_config=dict(type=vae_core, args=dict(in_features=7, **core)),
        decoder_config=dict(type=vae_core, args=dict(**core)),
        loss_config=dict(reconstruction_loss=dict(type="GraspReconstructionLoss"), latent_loss=dict(type="VAELatentLoss")),
        num_output_qualities=0, intermediate_feature_resolution=16)))
    ddm = dict(model=dict(type="GraspLatentDDM", args=dict(
        model=dict(type="TimeConditionedResNet1D", args=dict(
            dim=latent, channels=1, is_time_conditioned=True, learned_variance=False, learned_sinusoidal_cond=False,
            random_fourier_features=True, **rn)),
        latent_in_features=latent, diffusion_timesteps=1000, noise_scheduler_type=scheduler, diffusion_loss="l2",
        beta_schedule="linear", is_conditioned=True, joint_training=False, denoising_loss_weight=1,
        variance_type="fixed_large", elucidated_diffusion=False, beta_start=0.00005, beta_end=0.001)))
    return dict(vae=vae, ddm=ddm)


def build_fpc_ldm(n_points=1024, scheduler="ddim", seed=0, device=None, **kw):
    cfg = fpc_model_config(n_points, scheduler, **kw)
    ldm = build_model_from_cfg(cfg["ddm"])
    ldm.set_vae_model(build_model_from_cfg(cfg["vae"]))
    load_synthetic_weights(ldm, seed=seed)
    ldm.eval()
    return ldm.to(device) if device is not None else ldm



def classifier_model_config(n_cloud_points=1024, n_gripper_points=64, backbone="PVCNN", backbone_args=None):
    """A reference-style config of the grasp success classifier (grasp_classifier.py:18-52): `num_pc_points` counts the
    merged scene, cloud + gripper points; the backbone sees one extra feature channel, the cloud / gripper label."""
    if backbone == "PVCNN":
        args = dict(extra_feature_channels=1, scale_channels=0.25, scale_voxel_resolution=0.75, num_blocks=(1, 1, 1, 1))
    elif backbone == "PVCNN2":
        args = dict(extra_feature_channels=1)
    else:
        raise ValueError(f"backbone must be PVCNN or PVCNN2, not {backbone!r}")
    args.update(backbone_args or {})
    return dict(model=dict(type="PointsBasedGraspClassifier", args=dict(
        num_pc_points=n_cloud_points + n_gripper_points, points_backbone_config=dict(type=backbone, args=args),
        loss_config=dict(classification_loss=dict(type="BCEClassificationLoss", args={})))))


def build_classifier(n_cloud_points=1024, n_gripper_points=64, backbone="PVCNN", seed=0, device=None, backbone_args=None):
    model = build_model_from_cfg(classifier_model_config(n_cloud_points, n_gripper_points, backbone, backbone_args))
    load_synthetic_weights(model, seed=seed)
    model.eval()
    return model.to(device) if device is not None else model
