"""Drop-in replacements for the reference model classes (mask2former/utils/custom_model.py:18-53,
56-143, 324-390), with the v0.4.0 pixel-level body running on the HIP kernels.

Same class names, constructor signatures (``version`` kwarg), ``config_class``,
``main_input_name``, forward signatures, output dataclass and state_dict keys, so a
checkpoint of the reference loads unchanged.  Outside the hot path the model is the installed
Hugging Face Mask2Former with its modules swapped in place for the HIP ones of SURVEY §8(f):
Swin-T layers (f2), pixel-decoder deformable attention and encoder layers (f2), the masked-
attention decoder layers and mask predictor (f1), every nn.Linear / nn.LayerNorm (f1 / f2),
the loss's matcher costs, assignment and point-sampled mask terms (f3), and every convolution
(conv.HipConv2d: the pixel decoder's 1x1 input projections and mask projection, the FPN 3x3 and
Swin's 4x4 patch embedding as MFMA GEMMs, forward and backward).
"""
import contextlib
import random

import numpy as np
import torch
from torch import Tensor
from transformers import Mask2FormerConfig, Mask2FormerForUniversalSegmentation, Mask2FormerModel
from transformers.models.mask2former.modeling_mask2former import (Mask2FormerPixelLevelModule,
                                                                  Mask2FormerPixelLevelModuleOutput)

from . import deform_attn, dense, mask_predictor, masked_attention, ops, point_loss, swin
from .hot_path import float32_interface, hot_path, prepare
from .modules import DSAModule, DepthGradientInjectionResidual, EnhancedDepthImageRatioPredictor

SUPPORTED_VERSIONS = ("0.4.0", "0.0.0")


def set_seed(seed=42):
    """custom_model.py:18-25."""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)


class CustomConfig(Mask2FormerConfig):
    model_type = "mask2former"

    def __init__(self, attribute=1, **kwargs):
        self.attribute = attribute
        super().__init__(**kwargs)


class CustomMask2FormerPixelLevelModule(Mask2FormerPixelLevelModule):
    """v0.4.0: 10-channel input (RGB, depth x3, DGGM gradient x3, DGGM mask); version 0.0.0:
    plain RGB (the baseline branch, custom_model.py:145-146)."""
    main_input_name = "pixel_values"

    def __init__(self, config, version):
        super().__init__(config)
        if version not in SUPPORTED_VERSIONS:
            raise NotImplementedError(
                f"version {version!r}: only the paper model 0.4.0 (and the RGB baseline 0.0.0) are built "
                "MI355X-native; the abandoned variants of custom_model.py are out of scope (SURVEY §2 row 1x)")
        self.version = version
        # bf16 MFMA for the DSAM / ratio-predictor GEMMs; float32 is the exact parity mode
        self.compute_dtype = torch.float32
        # None: the hot path's colour maps / cp1 / features in the compute dtype; torch.float32 with
        # bf16 compute: the float32-interface mode (hot_path.float32_interface)
        self.interface_dtype = None
        # False: the reference's detached colour maps (Q1; the encoder takes no gradient).  True:
        # the opt-in end-to-end mode (set_end_to_end); 0.0.0 ignores it
        self.end_to_end = False
        if version == "0.4.0":
            self.ratio_predictor = EnhancedDepthImageRatioPredictor(3)
            self.dsam0 = DSAModule(in_channels=96, out_channels=192, num_depth_regions=3)
            self.dsam1 = DSAModule(in_channels=192, out_channels=384, num_depth_regions=3)
            self.dsam2 = DSAModule(in_channels=384, out_channels=768, num_depth_regions=3)
            self.depth_gradient_injection = DepthGradientInjectionResidual([96, 192, 384, 768], 3)

    def set_compute_dtype(self, dtype, interface=None):
        float32_interface(dtype, interface)
        self.compute_dtype = dtype
        self.interface_dtype = interface
        for m in self.modules():
            if hasattr(m, "compute_dtype"):
                m.compute_dtype = dtype
        return self

    def hot_path_features(self, pixel_values: Tensor, color_feature_map, ratios=None, status_sink=None,
                          color_grads=False):
        """custom_model.py:325-355 on the HIP kernels: returns the 4 backbone features.
        ``status_sink``: see hot_path.hot_path (None = raise the reference's ValueError at once).
        ``color_grads``: hot_path's end-to-end mode (the colour maps take gradients)."""
        # the ratio-free part (decomposition modes, bf16 colour layouts) beside the ratio predictor
        prep = prepare(pixel_values, list(color_feature_map), self.compute_dtype,
                       dsam_modules=[self.dsam0, self.dsam1, self.dsam2], interface_dtype=self.interface_dtype,
                       color_grads=color_grads)
        if ratios is None:
            ratios = self.ratio_predictor(pixel_values[:, 3:6])       # :336 (no grad, Q2)
        feats = hot_path(pixel_values, ratios, list(color_feature_map), [self.dsam0, self.dsam1, self.dsam2],
                         self.depth_gradient_injection, dtype=self.compute_dtype,
                         check_status=status_sink is None, status_sink=status_sink, prepared=prep,
                         interface_dtype=self.interface_dtype, color_grads=color_grads)
        dt = color_feature_map[0].dtype
        return [f.to(dt) for f in feats]

    def check_statuses(self):
        """After a replay of a captured step (its stream synchronised): raise the reference's
        ValueError for an image whose depth range the decomposition rejected."""
        for st in getattr(self, "captured_statuses", ()):
            st.check()

    def forward(self, pixel_values: Tensor, output_hidden_states: bool = False) -> Mask2FormerPixelLevelModuleOutput:
        if self.version == "0.0.0":
            backbone_features = list(self.encoder(pixel_values).feature_maps)
        else:
            rgb = pixel_values[:, 0:3, :, :]
            # :330 — Swin-T on the HIP layers (f2).  Its maps are detached at :332-333 (Q1), so no
            # graph is recorded for it: identical values, the fused forward-only kernels apply.
            # End-to-end mode (opt-in, a departure from Q1): the encoder records its graph and the
            # maps go to the hot path undetached, which returns their gradients.
            e2e = self.end_to_end and torch.is_grad_enabled()
            with contextlib.nullcontext() if e2e else torch.no_grad():
                color_feature_map = self.encoder(rgb).feature_maps
            statuses = []
            backbone_features = self.hot_path_features(pixel_values, color_feature_map, status_sink=statuses,
                                                       color_grads=e2e)
        with ops.host_constants():  # the pixel decoder's level-shape tensor (modeling_mask2former.py:1347)
            decoder_output = self.decoder(backbone_features, output_hidden_states=output_hidden_states)
        if self.version != "0.0.0":
            # The reference raises numpy's ValueError for a non-finite or too-narrow depth range
            # (custom_model.py:715-717).  The decomposition status was copied to the host behind
            # the decomposition; waiting for it here lets the DSAM / DGGM / pixel-decoder kernels
            # already enqueued keep the GPU busy.
            if ops.capturing():
                # a captured step: the statuses are read after each replay (check_statuses())
                self.captured_statuses = statuses
            else:
                for st in statuses:
                    st.check()
        return Mask2FormerPixelLevelModuleOutput(
            encoder_last_hidden_state=backbone_features[-1],
            encoder_hidden_states=tuple(backbone_features) if output_hidden_states else None,
            decoder_last_hidden_state=decoder_output.mask_features,
            decoder_hidden_states=decoder_output.multi_scale_features,
        )


class CustomMask2FormerModel(Mask2FormerModel):
    main_input_name = "pixel_values"

    def __init__(self, config, version):
        super().__init__(config)
        self.pixel_level_module = CustomMask2FormerPixelLevelModule(config, version=version)
        # f1: mask einsum + attention-mask binarisation of the masked-attention decoder on the
        # HIP kernels (class swap: parameters and state_dict keys unchanged)
        mask_predictor.install(self.transformer_module)
        # f1: the decoder layers' masked cross-attention core (scores, mask, softmax, P.V and its
        # backward) on the HIP kernels; torch's module path for inputs the kernels do not cover
        masked_attention.install(self.transformer_module)
        # f2: the pixel decoder's deformable-attention core on the fused HIP gather kernels
        deform_attn.install(self.pixel_level_module.decoder)
        # f1 / f2: the dense layers — every nn.Linear and nn.LayerNorm, the decoder and pixel-
        # decoder encoder layers (fused FFN), the Swin-T layers (window attention) — on the HIP
        # GEMM / LayerNorm / attention kernels
        swin.install(self.pixel_level_module.encoder)
        dense.install(self)


class CustomMask2FormerForUniversalSegmentation(Mask2FormerForUniversalSegmentation):
    main_input_name = "pixel_values"
    config_class = CustomConfig

    def __init__(self, config, version="0.0.0"):
        super().__init__(config)
        set_seed(42)                                                    # Q17: after HF init
        self.model = CustomMask2FormerModel(config, version=version)
        # f3: the loss's point-sampled mask terms and its matcher's costs on the HIP kernels, the
        # Hungarian assignments solved on the GPU (no host round trip)
        point_loss.install(self.criterion)
        # f1: the class head (built by the HF constructor after the model body was installed)
        dense.install(self.class_predictor)

    def set_compute_dtype(self, dtype, interface=None):
        self.model.pixel_level_module.set_compute_dtype(dtype, interface)
        return self

    def set_end_to_end(self, flag=True):
        """Opt into (or out of) the end-to-end mode of the paper model: the Swin encoder is no
        longer run under no_grad and its four maps take gradients through the fused hot path
        (DESIGN.md §5.17).  The default, False, is the reference's behaviour: detached colour maps
        (Q1), so no encoder parameter receives a gradient.  version="0.0.0" ignores the flag."""
        self.model.pixel_level_module.end_to_end = bool(flag)
        return self
