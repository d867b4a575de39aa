"""GraspCVAE (generation half): mirror of `grasp_ldm/models/grasp_vae.py` with the same
constructor arguments, sub-module names and state_dict keys (encoder.pc_encoder.*,
encoder.grasp_encoder.*, bottleneck.*, decoder.*).  Both directions run: cloud + latent -> pose (decoder) and
cloud + grasp -> latent (grasp encoder + bottleneck, one HIP launch: gldm_encode).  Losses are training-only."""
from typing import Union

import torch
from torch import nn

from .pc_encoders import PVCNN2Encoder, PVCNNEncoder
from .resnets import ResNet1D, Unet1D


def _get(cfg, key):
    return cfg[key] if isinstance(cfg, dict) else getattr(cfg, key)


def _rows_of(cond):
    """Rows of a conditioning latent: 0 for none (a Unet1D core without input conditioning), 1 for [n, Dc], R for [n, R, Dc]."""
    return 0 if cond is None else (1 if cond.ndim == 2 else cond.shape[1])


class ConditionalGraspPoseDecoder(nn.Module):
    """grasp_vae.py:353-436: Linear(D->R) -> ResNet1D -> tmrp(6) / class_logits(1), one HIP launch.  With a Unet1D core:
    in_layer, the fused Unet1D kernel, and the 7-row head as three launches (unet1d.UnetCoreEngine)."""
    MODELS = {"Unet1D": Unet1D, "ResNet1D": ResNet1D}

    def __init__(self, config, in_features, feature_resolution, num_output_qualities=None):
        super().__init__()
        if _get(config, "type") not in self.MODELS:
            raise NotImplementedError(f"Base network arch of type=`{_get(config, 'type')}` is not implemented. "
                                      f"Available base network types are: {list(self.MODELS)}")
        self.in_features, self.feature_resolution = in_features, feature_resolution
        self.in_layer = nn.Linear(in_features, feature_resolution)
        self.net = self.MODELS[_get(config, "type")](dim=feature_resolution, **dict(_get(config, "args")))
        self.tmrp = nn.Linear(self.net.out_features, 6)
        self.class_logits = nn.Linear(self.net.out_features, 1)
        self._use_qualities = bool(num_output_qualities is not None and num_output_qualities > 0)
        if self._use_qualities:
            raise NotImplementedError("quality heads (num_output_qualities > 0) are not on the shipped hot path")
        self.num_qualities = None
        self.out_features = (6, 1)
        self._engine = None   # the _cache.cached entry of _get_engine()

    def _pack(self, device, rows):
        sd = {k: v.detach().float().cpu() for k, v in self.state_dict().items()}
        if isinstance(self.net, Unet1D):
            from .unet1d import UnetCoreEngine
            self.net.cond_rows = rows
            return UnetCoreEngine.decoder(self.net.engine(device), sd)
        from .r1d import R1dEngine, pack_resnet1d
        packed = pack_resnet1d(sd, "net.", groups=self.net.groups, seq_len=self.feature_resolution,
                               cond_rows=rows, decoder=dict(
                                   in_w=sd["in_layer.weight"], in_b=sd["in_layer.bias"],
                                   tmrp_w=sd["tmrp.weight"], tmrp_b=sd["tmrp.bias"],
                                   cls_w=sd["class_logits.weight"], cls_b=sd["class_logits.bias"]))
        return R1dEngine(packed, device)

    def _get_engine(self, device, rows):
        from ._cache import cached, params_key
        return cached(self, "_engine", params_key(self.parameters(), device, rows), lambda: self._pack(device, rows), device,
                      required=True)

    @torch.no_grad()
    def forward(self, z_h, cond=None, samples_per_cond=1):
        if not z_h.is_cuda:
            raise RuntimeError("z_h must be a CUDA tensor (graspldm_amd has no CPU path)")
        eng = self._get_engine(z_h.device, _rows_of(cond))
        return eng.decode(z_h, eng.cond_embed(cond), samples_per_cond)


class ConditionalGraspPoseEncoder(nn.Module):
    """grasp_vae.py:439-536: Linear(D->R) -> ResNet1D -> Linear(R->L).  On the fused path (GraspCVAE.encode) the
    bottleneck's mu / logvar Linears ride on the same launch as the folded head (r1d_pack: encoder=).  With a Unet1D
    core the folded head is one launch behind the fused Unet1D kernel (unet1d.UnetCoreEngine)."""
    MODELS = {"Unet1D": Unet1D, "ResNet1D": ResNet1D}

    def __init__(self, config, latent_size, feature_resolution=16):
        super().__init__()
        assert _get(config, "type") in self.MODELS, (
            f"Cannot build GraspPoseEncoder of model_type: {_get(config, 'type')} from supported models: {self.MODELS}")
        args = dict(_get(config, "args"))
        self.in_features = args.pop("in_features")
        self.out_features = latent_size
        self.feature_resolution = feature_resolution
        self.in_layer = nn.Linear(self.in_features, feature_resolution)
        self.net = self.MODELS[_get(config, "type")](dim=feature_resolution, **args)
        self.out_layer = nn.Linear(self.net.out_features, self.out_features)
        self._engine = None         # _cache.cached entries of _get_engine(): fused with a bottleneck,
        self._engine_plain = None   # and out_layer only (forward() on its own)

    def _pack(self, device, rows, bottleneck):
        from .r1d import R1dEngine, pack_resnet1d
        sd = {k: v.detach().float().cpu() for k, v in self.state_dict().items()}
        if isinstance(self.net, Unet1D):
            from .unet1d import UnetCoreEngine
            self.net.cond_rows = rows
            bn = {k: v.detach().float().cpu() for k, v in bottleneck.state_dict().items()} if bottleneck is not None else None
            return UnetCoreEngine.encoder(self.net.engine(device), sd, bn)
        lz = self.out_features
        if bottleneck is not None:
            bn = {k: v.detach().float().cpu() for k, v in bottleneck.state_dict().items()}
            head = dict(mu_w=bn["mu.weight"], mu_b=bn["mu.bias"], logvar_w=bn["logvar.weight"], logvar_b=bn["logvar.bias"])
        else:   # identity bottleneck: mu = out_layer's output
            head = dict(mu_w=torch.eye(lz), mu_b=torch.zeros(lz), logvar_w=torch.eye(lz), logvar_b=torch.zeros(lz))
        packed = pack_resnet1d(sd, "net.", groups=self.net.groups, seq_len=self.feature_resolution, cond_rows=rows,
                               encoder=dict(in_w=sd["in_layer.weight"], in_b=sd["in_layer.bias"],
                                            out_w=sd["out_layer.weight"], out_b=sd["out_layer.bias"], **head))
        return R1dEngine(packed, device)

    def _get_engine(self, device, rows, bottleneck=None):
        from ._cache import cached, params_key
        params = list(self.parameters()) + (list(bottleneck.parameters()) if bottleneck is not None else [])
        return cached(self, "_engine" if bottleneck is not None else "_engine_plain", params_key(params, device, rows),
                      lambda: self._pack(device, rows, bottleneck), device, required=True)

    @torch.no_grad()
    def forward(self, x, cond, samples_per_cond=1):
        """x [n,1,D], cond [n / samples_per_cond, R, Dc] -> [n,1,L] (grasp_vae.py:518-536)."""
        if not x.is_cuda:
            raise RuntimeError("x must be a CUDA tensor (graspldm_amd has no CPU path)")
        eng = self._get_engine(x.device, _rows_of(cond))
        out, _, _ = eng.encode(x.reshape(x.shape[0], -1), eng.cond_embed(cond), samples_per_cond, want_z=False)
        return out.unsqueeze(-2)


class VAEBottleneck(nn.Module):
    """grasp_vae.py:539-574.  On their own these are two tiny Linears (plain torch on the tensor's device); the fused
    path (GraspCVAE.encode) never calls them."""

    def __init__(self, in_features, latent_size):
        super().__init__()
        self.mu = nn.Linear(in_features, latent_size)
        self.logvar = nn.Linear(in_features, latent_size)

    def reparameterize(self, mu, logvar):
        std = torch.exp(0.5 * logvar)
        eps = torch.randn(std.shape).to(std.device)   # CPU generator, then moved (the rule generate_grasps follows)
        return mu + eps * std

    @torch.no_grad()
    def forward(self, z):
        return self.mu(z), self.logvar(z)


class PcConditionedGraspEncoder(nn.Module):
    """grasp_vae.py:258-350"""
    PC_ENCODERS = {"PVCNNEncoder": PVCNNEncoder, "PVCNN2Encoder": PVCNN2Encoder}

    def __init__(self, pc_encoder_config, grasp_encoder_config, pc_latent_size=64, grasp_latent_size=4):
        super().__init__()
        t = _get(pc_encoder_config, "type")
        if t not in self.PC_ENCODERS:
            raise NotImplementedError(f"Pointcloud encoder network arch of type=`{t}` is not implemented. "
                                      f"Available base network types are: {list(self.PC_ENCODERS)}")
        self.pc_encoder = self.PC_ENCODERS[t](out_features=pc_latent_size, **dict(_get(pc_encoder_config, "args")))
        self.grasp_encoder = ConditionalGraspPoseEncoder(config=grasp_encoder_config, latent_size=grasp_latent_size)
        self.out_features = grasp_latent_size

    def encode_pc(self, xyz):
        return self.pc_encoder(xyz)

    def get_conditioning_latent(self, xyz):
        return self.encode_pc(xyz)

    @torch.no_grad()
    def forward(self, xyz, h, z_pc=None):
        """grasp_vae.py:305-344: (z_grasp [n,1,L], z_pc [n,R,Dc] repeated per grasp).  A given z_pc is taken as the
        reference takes it: already one row block per grasp."""
        if not h.is_cuda:
            raise RuntimeError("h must be a CUDA tensor (graspldm_amd has no CPU path)")
        if z_pc is not None:
            return self.grasp_encoder(h.unsqueeze(1), cond=z_pc), z_pc
        reps = h.shape[0] // xyz.shape[0]
        z = self.pc_encoder(xyz)
        return self.grasp_encoder(h.unsqueeze(1), cond=z, samples_per_cond=reps), z.repeat_interleave(reps, dim=0)


class GraspCVAE(nn.Module):
    """grasp_vae.py:17-255"""

    def __init__(self, grasp_latent_size: int, pc_latent_size: int, grasp_encoder_config: dict,
                 pc_encoder_config: dict, decoder_config: dict, loss_config: dict = None,
                 intermediate_feature_resolution: int = 16, num_output_qualities: Union[int, None] = None) -> None:
        super().__init__()
        self.grasp_latent_size, self.pc_latent_size = grasp_latent_size, pc_latent_size
        self.loss_config = loss_config  # accepted and ignored: losses are training-only (grasp_vae.py:55-69)
        self.encoder = PcConditionedGraspEncoder(pc_encoder_config=pc_encoder_config,
                                                 grasp_encoder_config=grasp_encoder_config,
                                                 pc_latent_size=pc_latent_size, grasp_latent_size=grasp_latent_size)
        self.bottleneck = VAEBottleneck(in_features=self.encoder.out_features, latent_size=grasp_latent_size)
        self.num_output_qualities = num_output_qualities
        self.decoder = ConditionalGraspPoseDecoder(in_features=grasp_latent_size, config=decoder_config,
                                                   num_output_qualities=num_output_qualities,
                                                   feature_resolution=intermediate_feature_resolution)
        self.out_features = self.decoder.out_features

    @property
    def use_grasp_qualities(self) -> bool:
        return bool(self.decoder._use_qualities)

    def encode_pc(self, xyz):
        return self.encoder.encode_pc(xyz)

    def sample_grasp_latent(self, batch_size, device):
        return torch.randn(batch_size, self.grasp_latent_size).to(device)

    @torch.no_grad()
    def generate_grasps(self, xyz, num_grasps=10, z_h=None):
        """grasp_vae.py:226-255: encode cloud -> N(0,I) latents (CPU generator, then moved) -> decode.
        The cloud latent is shared by index (sample i -> cloud i // num_grasps) instead of
        materialising repeat_interleave."""
        assert xyz.ndim == 3, (f"Input pointcloud should be  3-dim tensor of shape [B, N, 3]. "
                               f"Found a {xyz.ndim} dimensional tensor.")
        z_pc = self.encode_pc(xyz)
        if z_h is None:
            z_h = torch.randn(xyz.shape[0] * num_grasps, self.grasp_latent_size)
        return self.decoder(z_h.to(xyz.device), z_pc, samples_per_cond=num_grasps)

    @torch.no_grad()
    def _encode(self, xyz, grasp, eps=None, mix=(1.0, 1.0), eps_times_std=True, want_z=True):
        """One cloud-encoder pass, one cond_embed, one gldm_encode -> (mu, logvar, z, z_pc [B,R,Dc], grasps per cloud).
        The cloud latent is shared by index (grasp i -> cloud i // G), like the decoder does."""
        if not (xyz.is_cuda and grasp.is_cuda):
            raise RuntimeError("xyz and grasp must be CUDA tensors (graspldm_amd has no CPU path)")
        assert xyz.ndim == 3, (f"Input pointcloud should be  3-dim tensor of shape [B, N, 3]. "
                               f"Found a {xyz.ndim} dimensional tensor.")
        n, b = grasp.shape[0], xyz.shape[0]
        if n % b:
            raise RuntimeError(f"{n} grasps do not split over {b} clouds")
        z_pc = self.encode_pc(xyz)
        ge = self.encoder.grasp_encoder
        eng = ge._get_engine(xyz.device, _rows_of(z_pc), self.bottleneck)
        mu, logvar, z = eng.encode(grasp, eng.cond_embed(z_pc), n // b, eps=eps, mix=mix, eps_times_std=eps_times_std,
                                   want_z=want_z)
        return mu, logvar, z, z_pc, n // b

    @torch.no_grad()
    def encode(self, xyz, grasp, eps=None):
        """grasp_vae.py:104-117 -> ((mu, logvar, z), (None, None, z_pc)).  eps [B*G, L] (additive): the normals of the
        reparameterisation; None draws them on the CPU generator and moves them, so torch.manual_seed reproduces the
        reference's randn_like stream.  z_pc comes back repeated per grasp [B*G, R, Dc] as in the reference."""
        if not (xyz.is_cuda and grasp.is_cuda):
            raise RuntimeError("xyz and grasp must be CUDA tensors (graspldm_amd has no CPU path)")
        if eps is None:
            eps = torch.randn(grasp.shape[0], self.grasp_latent_size)
        mu, logvar, z, z_pc, g = self._encode(xyz, grasp, eps=eps.to(xyz.device))
        return (mu, logvar, z), (None, None, z_pc.repeat_interleave(g, dim=0))

    def forward(self, xyz, grasp, compute_loss=True, eps=None, **kwargs):
        """grasp_vae.py:119-147.  compute_loss=False: encode -> reparameterise -> decode, (tmrp, logit).  The losses are
        training (compute_loss=True, the reference's default, raises)."""
        if compute_loss:
            raise NotImplementedError("VAE losses are training-only (out of scope): call forward(xyz, grasp, "
                                      "compute_loss=False) for the reconstruction")
        if not (xyz.is_cuda and grasp.is_cuda):
            raise RuntimeError("xyz and grasp must be CUDA tensors (graspldm_amd has no CPU path)")
        if eps is None:
            eps = torch.randn(grasp.shape[0], self.grasp_latent_size)
        _, _, z, z_pc, g = self._encode(xyz, grasp, eps=eps.to(xyz.device))
        return self.decoder(z, z_pc, samples_per_cond=g)
