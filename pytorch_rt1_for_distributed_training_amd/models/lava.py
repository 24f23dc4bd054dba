"""LAVA (Language-Attends-to-Vision-to-Act) behaviour-cloning policy -- the second model family.

Behavioural spec: ``language_table/train/networks/{lava,dense_resnet}.py`` and the
``language_table_sim_local`` config (sequence 4, d_model 128, 2 heads, 4 pixel-language layers, 2 temporal
layers, pyramid levels (2, 3, 4), conv-maxpool image encoder, dense-resnet head 1024 x 2 blocks, MSE BC):

  rgb (B, T, H, W, 3) -> conv3x3+ReLU+maxpool x4 (+1 maxpool) feature pyramid
  -> per chosen level: Dense -> d_model, * sqrt(d_model), + 2-D sin/cos positions -> one "visual sentence"
  -> language query (512-d instruction embedding -> Dense -> d_model, * sqrt(d_model)) attends to the visual
     sentence through pre-norm cross-attention layers (residual on the language path only, ReLU FFN)
  -> LayerNorm -> temporal pre-norm transformer over the T steps (+ 1-D sin/cos positions), mean over time, LN
  -> dense resnet -> action (2).
Dense layers use N(0, 0.05) kernel and bias init as in the reference.  The language encoder is the
``clip_in_obs`` variant: a precomputed 512-d embedding per step (here from any text encoder, e.g.
``sim.HashedTextEncoder``) -- the frozen CLIP text tower and its checkpoint are not available offline.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F


@dataclass
class LavaConfig:
    sequence_length: int = 4
    d_model: int = 128
    num_heads: int = 2
    num_layers: int = 4                       # pixel-language layers
    temporal_layers: int = 2
    pyramid_fuse_layers: Tuple[int, ...] = (2, 3, 4)
    dense_resnet_width: int = 1024
    dense_resnet_blocks: int = 2
    action_size: int = 2
    lang_dim: int = 512
    height: int = 180
    width: int = 320
    dropout: float = 0.1
    backend: str = "torch"                    # pixel-language attention: torch | hip | auto (ops/lava_attention.py)
    encoder_backend: str = "torch"            # conv-maxpool image encoder: torch | hip | auto (ops/lava_conv.py)
    sentence_backend: str = "torch"           # level projections -> pixels: torch | hip | auto (ops/lava_sentence.py)
    language_backend: str = "torch"           # cross layers' language rows: torch | hip | auto (ops/lava_language.py)
    head_backend: str = "torch"               # dense resnet + action projection: torch | hip | auto (ops/lava_head.py)


def _dense(i: int, o: int) -> nn.Linear:
    lin = nn.Linear(i, o)
    nn.init.normal_(lin.weight, std=0.05)
    nn.init.normal_(lin.bias, std=0.05)
    return lin


def _flax_conv(cin: int, cout: int, k: int) -> nn.Conv2d:
    """3x3 SAME conv with Flax ``nn.Conv``'s default init (``pixel.py:56``): truncated LeCun-normal weights
    (variance 1 / fan_in, truncated at 2 sigma) and a zero bias."""
    conv = nn.Conv2d(cin, cout, k, padding=k // 2)
    std = math.sqrt(1.0 / (cin * k * k)) / 0.87962566103423978
    nn.init.trunc_normal_(conv.weight, std=std, a=-2 * std, b=2 * std)
    nn.init.zeros_(conv.bias)
    return conv


def sincos_1d(length: int, d: int) -> torch.Tensor:
    pe = np.zeros((length, d), np.float32)
    pos = np.arange(length)[:, None]
    div = np.exp(np.arange(0, d, 2) * -(np.log(1.0e4) / d))
    pe[:, 0::2] = np.sin(pos * div)
    pe[:, 1::2] = np.cos(pos * div)
    return torch.from_numpy(pe)


def sincos_2d(d: int, h: int, w: int) -> torch.Tensor:
    """(h*w, d): first half of the channels encodes the column, second half the row (sin/cos interleaved)."""
    if d % 4:
        raise ValueError("2-D sin/cos positions need d_model % 4 == 0")
    half = d // 2
    div = np.exp(np.arange(0.0, half, 2) * -(np.log(10000.0) / half))
    pe = np.zeros((d, h, w), np.float32)
    px = np.arange(w)[:, None] * div                                     # (w, half/2)
    py = np.arange(h)[:, None] * div
    pe[0:half:2] = np.sin(px).T[:, None, :]
    pe[1:half:2] = np.cos(px).T[:, None, :]
    pe[half::2] = np.sin(py).T[:, :, None]
    pe[half + 1::2] = np.cos(py).T[:, :, None]
    return torch.from_numpy(pe.reshape(d, h * w).T.copy())


class ConvMaxpoolEncoder(nn.Module):
    """Feature pyramid: 4 x (conv3x3 SAME + ReLU + maxpool2), then one more maxpool (5 levels).  The convs take
    Flax ``nn.Conv``'s default init like the reference's (``language_table/train/networks/lava.py:43``)."""

    def __init__(self, channels: Sequence[int] = (32, 64, 128, 256), backend: str = "torch"):
        super().__init__()
        convs, cin = [], 3
        for c in channels:
            convs.append(_flax_conv(cin, c, 3))
            cin = c
        self.convs = nn.ModuleList(convs)
        self.channels = list(channels) + [channels[-1]]
        self.backend = "torch"
        if backend != "torch":
            from ..ops.lava_conv import resolve_backend
            stages = tuple(zip([3] + list(channels[:-1]), channels))
            self.backend = resolve_backend(backend, stages)              # ValueError when hip cannot be served

    def forward(self, x):                  # torch: x (N, 3, H, W); hip: the frames (N, H, W, 3), uint8 or fp32
        if self.backend == "hip":
            # conv + bias + ReLU + pool per stage in one MFMA kernel, NHWC bf16 between the stages (lavaconv.hip);
            # a level is the logical (N, C, h, w) fp32 view of that storage
            from ..ops.lava_conv import conv_relu_pool
            levels = []
            for conv in self.convs:
                x = conv_relu_pool(x, conv)
                levels.append(x.permute(0, 3, 1, 2).float())
            levels.append(F.max_pool2d(levels[-1], 2))
            return levels
        levels = []
        for conv in self.convs:
            x = F.max_pool2d(F.relu(conv(x)), 2)
            levels.append(x)
        levels.append(F.max_pool2d(x, 2))
        return levels

    def stages_nhwc(self, x):              # hip only: the four stage outputs as the kernels store them, NHWC bf16
        if self.backend != "hip":
            raise ValueError("the NHWC bf16 stage outputs exist only on the hip encoder backend")
        from ..ops.lava_conv import conv_relu_pool
        stages = []
        for conv in self.convs:
            x = conv_relu_pool(x, conv)
            stages.append(x)
        return stages


class CrossLayer(nn.Module):
    """Pre-norm language(query) -> pixels(key/value) attention with a residual on the language path."""

    def __init__(self, d: int, heads: int, dff: int, dropout: float, backend: str = "torch",
                 language_backend: str = "torch"):
        super().__init__()
        self.ln_pix, self.ln_lang, self.ln_ffn = nn.LayerNorm(d), nn.LayerNorm(d), nn.LayerNorm(d)
        self.attn = nn.MultiheadAttention(d, heads, batch_first=True)
        self.ff1, self.ff2 = _dense(d, dff), _dense(dff, dff)
        self.drop = nn.Dropout(dropout)
        self.backend = backend                                           # "torch" or "hip", already resolved
        self.language_backend = language_backend                         # likewise; "hip" needs backend "hip"

    def forward(self, pix, lang):
        if self.language_backend == "hip":
            # ln_lang, then everything after the attention in one launch (lavalang.hip); a stack of layers goes
            # through cross_stack as a whole, which also folds the next layer's ln_lang into this one's launch
            from ..ops.lava_language import cross_stack
            return cross_stack(pix, lang[:, 0], [self])[0][:, None]
        if self.backend == "hip":
            # pixel LayerNorm, K / V projections and the one-query attention in one pass over pix (lavaxattn.hip);
            # the out-projection, dropout and FFN are [N, d] work and stay as they are
            from ..ops.lava_attention import cross_attention
            ctx = cross_attention(pix, self.ln_lang(lang)[:, 0], self.ln_pix, self.attn)
            x3 = lang + self.drop(self.attn.out_proj(ctx)[:, None])
            return x3 + self.drop(self.ff2(F.relu(self.ff1(self.ln_ffn(x3)))))
        p, q = self.ln_pix(pix), self.ln_lang(lang)
        x3 = lang + self.drop(self.attn(q, p, p, need_weights=False)[0])
        return x3 + self.drop(self.ff2(F.relu(self.ff1(self.ln_ffn(x3)))))


class SelfLayer(nn.Module):
    def __init__(self, d: int, heads: int, dff: int, dropout: float):
        super().__init__()
        self.ln1, self.ln2 = nn.LayerNorm(d), nn.LayerNorm(d)
        self.attn = nn.MultiheadAttention(d, heads, batch_first=True)
        self.ff1, self.ff2 = _dense(d, dff), _dense(dff, dff)
        self.drop = nn.Dropout(dropout)

    def forward(self, x):
        h = self.ln1(x)
        x3 = x + self.drop(self.attn(h, h, h, need_weights=False)[0])
        return x3 + self.drop(self.ff2(F.relu(self.ff1(self.ln2(x3)))))


class DenseResnet(nn.Module):
    def __init__(self, din: int, width: int, blocks: int):
        super().__init__()
        self.backend = "torch"                                           # "hip": set, resolved, by the model that owns
                                                                         # this and the projection (_resolve_head)
        self.inp = _dense(din, width)
        self.blocks = nn.ModuleList(nn.Sequential(nn.ReLU(), _dense(width, width // 4), nn.ReLU(),
                                                  _dense(width // 4, width // 4), nn.ReLU(),
                                                  _dense(width // 4, width)) for _ in range(blocks))

    def forward(self, x):
        if self.backend == "hip":
            # one launch per linear each way, ReLUs and the residual in their prologues and epilogues (lavahead.hip)
            from ..ops.lava_head import dense_resnet
            return dense_resnet(x, self)
        x = self.inp(x)
        for b in self.blocks:
            x = x + b(x)
        return x


def _resolve_head(backend: str, head: DenseResnet, action_projection: nn.Linear) -> str:
    """``torch | hip | auto`` -> ``torch | hip`` for a dense resnet and its action projection."""
    if backend == "torch":
        return "torch"
    from ..ops.lava_head import resolve_backend                          # ValueError when hip cannot be served
    return resolve_backend(backend, head.inp.in_features, head.inp.out_features, action_projection.out_features)


def policy_head(x, head: DenseResnet, action_projection: nn.Linear):
    """``action_projection(head(x))``; on hip the projection is the head's last kernel (lavahead.hip)."""
    if head.backend == "hip":
        from ..ops.lava_head import dense_resnet_head
        return dense_resnet_head(x, head, action_projection)
    return action_projection(head(x))


class SequenceLAVMSE(nn.Module):
    """obs {rgb (B,T,H,W,3) in [0,1] or uint8, instruction_embedding (B,T,512)} -> action (B, action_size)."""

    def __init__(self, cfg: LavaConfig = LavaConfig()):
        super().__init__()
        self.cfg = cfg
        d = cfg.d_model
        self.image_encoder = ConvMaxpoolEncoder(backend=cfg.encoder_backend)
        self.visual_proj = nn.ModuleDict({str(i): _dense(self.image_encoder.channels[i], d)
                                          for i in cfg.pyramid_fuse_layers})
        self.lang_proj = _dense(cfg.lang_dim, d)
        self.backend = "torch"
        if cfg.backend != "torch":
            from ..ops.lava_attention import resolve_backend
            self.backend = resolve_backend(cfg.backend, d, 2)            # ValueError when hip cannot be served
        self.sentence_backend = self._resolve_sentence(cfg)
        self.language_backend = self._resolve_language(cfg)
        self.cross = nn.ModuleList(CrossLayer(d, 2, d, cfg.dropout, self.backend, self.language_backend)
                                   for _ in range(cfg.num_layers))
        self.fuse_norm = nn.LayerNorm(d)
        self.temporal_in = _dense(d, d)
        self.temporal = nn.ModuleList(SelfLayer(d, cfg.num_heads, d, cfg.dropout)
                                      for _ in range(cfg.temporal_layers))
        self.temporal_norm = nn.LayerNorm(d)
        self.head = DenseResnet(d, cfg.dense_resnet_width, cfg.dense_resnet_blocks)
        self.action_projection = _dense(cfg.dense_resnet_width, cfg.action_size)
        self.head.backend = _resolve_head(cfg.head_backend, self.head, self.action_projection)
        self.drop = nn.Dropout(cfg.dropout)
        self.register_buffer("pos_t", sincos_1d(cfg.sequence_length, d), persistent=False)
        self._pos2d = {}

    def _resolve_sentence(self, cfg: LavaConfig) -> str:
        """``hip`` consumes the hip encoder's NHWC bf16 outputs and serves fuse levels (2, 3, 4) at d_model 128."""
        if cfg.sentence_backend == "torch":
            return "torch"
        from ..ops.lava_sentence import D_MODEL, FUSE_LAYERS, resolve_backend
        missing = None
        if self.image_encoder.backend != "hip":
            missing = "the hip sentence backend needs the hip encoder backend (encoder_backend='hip')"
        elif tuple(cfg.pyramid_fuse_layers) != FUSE_LAYERS:
            missing = (f"the hip sentence backend serves pyramid_fuse_layers == {FUSE_LAYERS}, "
                       f"got {tuple(cfg.pyramid_fuse_layers)}")
        elif cfg.d_model != D_MODEL:
            missing = f"the hip sentence backend serves d_model == {D_MODEL}, got {cfg.d_model}"
        if missing is None:
            return resolve_backend(cfg.sentence_backend, [self.image_encoder.channels[i] for i in FUSE_LAYERS],
                                   cfg.d_model)
        if cfg.sentence_backend == "auto":
            return "torch"
        resolve_backend(cfg.sentence_backend)                           # an unknown name or a missing GPU comes first
        raise ValueError(missing)

    def _resolve_language(self, cfg: LavaConfig) -> str:
        """``hip`` consumes the hip attention kernels' per-frame outputs, so it needs ``backend`` resolved to hip."""
        if cfg.language_backend == "torch":
            return "torch"
        from ..ops.lava_language import resolve_backend
        if self.backend == "hip":
            return resolve_backend(cfg.language_backend, cfg.d_model, cfg.d_model, 2)
        if cfg.language_backend == "auto":
            return "torch"
        resolve_backend(cfg.language_backend, cfg.d_model, cfg.d_model, 2)   # an unknown name or a missing GPU comes first
        raise ValueError("the hip language backend needs the hip attention backend (backend='hip')")

    def _pos_sentence(self, shapes, device) -> torch.Tensor:
        key = (tuple(shapes), str(device))
        if key not in self._pos2d:
            self._pos2d[key] = torch.cat([self._pos(h, w, device) for h, w in shapes], 0).contiguous()
        return self._pos2d[key]

    def _pos(self, h: int, w: int, device) -> torch.Tensor:
        key = (h, w, str(device))
        if key not in self._pos2d:
            self._pos2d[key] = sincos_2d(self.cfg.d_model, h, w).to(device)
        return self._pos2d[key]

    def encode(self, rgb: torch.Tensor, lang: torch.Tensor) -> torch.Tensor:
        b, t = rgb.shape[:2]
        x = rgb.reshape(b * t, *rgb.shape[2:])
        if self.image_encoder.backend == "hip":
            if x.dtype != torch.uint8:
                x = x.float()
        else:                                                           # the kernels read NHWC and fuse the /255
            if x.dtype == torch.uint8:
                x = x.float() / 255.0
            x = x.permute(0, 3, 1, 2).contiguous()                     # NHWC -> NCHW
        d = self.cfg.d_model
        if self.sentence_backend == "hip":
            # projections, scale, positions, cat and dropout in one MFMA kernel over the NHWC bf16 stage outputs
            # (lavasent.hip); level 4 is pooled from level 3 inside it
            from ..ops.lava_sentence import visual_sentence
            l2, l3 = self.image_encoder.stages_nhwc(x)[2:4]
            (h2, w2), (h3, w3) = l2.shape[1:3], l3.shape[1:3]
            pos = self._pos_sentence(((h2, w2), (h3, w3), (h3 // 2, w3 // 2)), l2.device)
            pixels = visual_sentence(l2, l3, self.visual_proj, pos, self.cfg.dropout, self.training)
        else:
            levels = self.image_encoder(x)
            sent = []
            for i in self.cfg.pyramid_fuse_layers:
                f = levels[i]                                           # (N, C, h, w)
                h, w = f.shape[-2:]
                v = self.visual_proj[str(i)](f.flatten(2).transpose(1, 2)) * math.sqrt(d)
                sent.append(v + self._pos(h, w, v.device))
            pixels = self.drop(torch.cat(sent, dim=1))                  # (N, sum hw, d)
        q = self.drop(self.lang_proj(lang.reshape(b * t, -1).to(self.lang_proj.weight.dtype)) * math.sqrt(d))[:, None]
        if self.language_backend == "hip":
            # the whole cross stack's language rows on lavalang.hip; the last layer's launch carries fuse_norm
            from ..ops.lava_language import cross_stack
            z = cross_stack(pixels, q[:, 0], self.cross, self.fuse_norm)[1].reshape(b, t, d)
        else:
            for layer in self.cross:
                q = layer(pixels, q)
            z = self.fuse_norm(q[:, 0]).reshape(b, t, d)
        z = self.temporal_in(z) * math.sqrt(d) + self.pos_t[:t]
        z = self.drop(z)
        for layer in self.temporal:
            z = layer(z)
        return self.temporal_norm(z.mean(dim=1))

    def forward(self, obs) -> torch.Tensor:
        return policy_head(self.encode(obs["rgb"], obs["instruction_embedding"]), self.head, self.action_projection)


# ---------------------------------------------------------------------------------------------------------------
# PixelLangMSE: the simple pixel-language BC network (reference language_table/train/networks/pixel.py:25-111)
class LanguageFusion(nn.Module):
    """Multiplicative language fusion: Dense(lang -> C) tiled over H x W, times the feature map."""

    def __init__(self, lang_dim: int, channels: int):
        super().__init__()
        self.proj = _dense(lang_dim, channels)

    def forward(self, lang, image):                                      # lang (B, D), image (B, C, H, W)
        return image * self.proj(lang)[:, :, None, None]


class ConvMaxpoolLanguageEncoder(nn.Module):
    """4 x [conv3x3 SAME (+bias) -> language fusion from the 2nd conv on -> ReLU -> maxpool 2 VALID], spatial
    mean, a final multiplicative language gate, ReLU, LayerNorm (``pixel.py:47-80``, ``fuse_from = 2``).

    ``backend`` ``hip`` (``ops/lava_pixel.py``) runs the convs, gates, ReLUs, pools and the tail on HIP kernels; the
    gate projections stay ``nn.Linear``.  It serves ``fuse_from == 2``, channels (32, 64, 128, 256) and 3, 6, 9 or 12
    stacked input channels; the parameters are the same on both backends."""

    def __init__(self, in_ch: int, lang_dim: int = 512, channels: Sequence[int] = (32, 64, 128, 256),
                 fuse_from: int = 2, backend: str = "torch"):
        super().__init__()
        self.backend = self._resolve(backend, in_ch, tuple(channels), fuse_from)
        convs, fuses, cin = [], [], in_ch
        for i, c in enumerate(channels):
            convs.append(_flax_conv(cin, c, 3))
            fuses.append(LanguageFusion(lang_dim, c) if fuse_from <= i + 1 else None)
            cin = c
        self.convs = nn.ModuleList(convs)
        self.fuses = nn.ModuleList(f if f is not None else nn.Identity() for f in fuses)
        self._fuse = [f is not None for f in fuses]
        self.lang_gate = _dense(lang_dim, channels[-1]) if fuse_from <= len(channels) + 1 else None
        self.norm = nn.LayerNorm(channels[-1], eps=1e-6)

    @staticmethod
    def _resolve(backend: str, in_ch: int, channels, fuse_from: int) -> str:
        if backend == "torch":
            return "torch"
        from ..ops.lava_conv import FIRST_STAGE_CIN
        from ..ops.lava_pixel import CHANNELS, resolve_backend
        missing = None
        if fuse_from != 2:
            missing = f"the hip pixel encoder serves fuse_from == 2, got {fuse_from}"
        elif channels != CHANNELS:
            missing = f"the hip pixel encoder serves channels {CHANNELS}, got {channels}"
        elif in_ch not in FIRST_STAGE_CIN:
            missing = (f"the hip pixel encoder is served for 3 * sequence_length in {FIRST_STAGE_CIN} stacked "
                       f"channels, got {in_ch}")
        if missing is None:
            return resolve_backend(backend, in_ch, channels)             # ValueError when hip cannot be served
        if backend == "auto":
            return "torch"
        resolve_backend(backend)                                         # an unknown name or a missing GPU comes first
        raise ValueError(missing)

    def forward(self, x, lang):            # torch: x (B, C, H, W); hip: the stacked frames (B, H, W, C), uint8 or fp32
        if self.backend == "hip":
            # per stage one MFMA kernel: conv + bias, the language gate, ReLU and pool in its epilogue, NHWC bf16
            # between the stages (lavaconv.hip); mean, final gate, ReLU and LayerNorm in one launch (lavapix.hip)
            from ..ops.lava_conv import conv_relu_pool, gated_conv_relu_pool
            from ..ops.lava_pixel import pixel_tail
            x = conv_relu_pool(x, self.convs[0])
            for conv, fuse in zip(self.convs[1:], self.fuses[1:]):
                x = gated_conv_relu_pool(x, conv, fuse.proj(lang))
            return pixel_tail(x, self.lang_gate(lang), self.norm)
        for conv, fuse, on in zip(self.convs, self.fuses, self._fuse):
            x = conv(x)
            if on:
                x = fuse(lang, x)
            x = F.max_pool2d(F.relu(x), 2)
        x = x.mean(dim=(2, 3))
        if self.lang_gate is not None:
            x = x * self.lang_gate(lang)
        return self.norm(F.relu(x))


class PixelLangMSE(nn.Module):
    """obs {rgb (B, N, W, H, C) in [0,1] or uint8, clip_embedding / instruction_embedding (B, N, 512)}
    -> action (B, action_size).

    The N frames are stacked channel-wise with the reference's raw reshape ``(b, n, w, h, c) -> (b, w, h, c*n)``
    (a reinterpretation of memory, not a transpose -- kept as is), the last step's language embedding conditions
    the encoder, then the dense resnet and an N(0, 0.05)-initialised action projection (``pixel.py:84-111``)."""

    def __init__(self, action_size: int = 2, dense_resnet_width: int = 1024, dense_resnet_num_blocks: int = 2,
                 sequence_length: int = 4, lang_dim: int = 512, head_backend: str = "torch",
                 encoder_backend: str = "torch"):
        super().__init__()
        self.encoder = ConvMaxpoolLanguageEncoder(3 * sequence_length, lang_dim, backend=encoder_backend)
        self.dense_resnet = DenseResnet(256, dense_resnet_width, dense_resnet_num_blocks)
        self.action_projection = _dense(dense_resnet_width, action_size)
        self.dense_resnet.backend = _resolve_head(head_backend, self.dense_resnet, self.action_projection)

    def forward(self, obs) -> torch.Tensor:
        rgb = obs["rgb"]
        hip = self.encoder.backend == "hip"                              # the kernels read NHWC and fuse the /255
        if rgb.dtype == torch.uint8:
            if not hip:
                rgb = rgb.float() / 255.0
        elif hip:
            rgb = rgb.float()
        b, n, w, h, c = rgb.shape
        rgb = rgb.contiguous().reshape(b, w, h, c * n)                  # reference's channel stacking
        lang = obs.get("clip_embedding", obs.get("instruction_embedding"))[:, -1]
        dtype = next(self.encoder.parameters()).dtype                    # fp32; fp64 in a .double() copy
        x = self.encoder(rgb if hip else rgb.permute(0, 3, 1, 2), lang.to(dtype))
        return policy_head(x, self.dense_resnet, self.action_projection)
