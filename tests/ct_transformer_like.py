"""A torch module with FunASR's CT-Transformer parameter names (embed, encoder.encoders0.0, encoder.encoders.N, self_attn.linear_q_k_v,
self_attn.fsmn_block, self_attn.linear_out, feed_forward.w_1 / w_2, encoder.after_norm, decoder) for both converter routes
(tests/test_punc_cpu.py): its state dict is the `.pt` route's input and its export the ONNX route's.  The blocks are
tests/funasr_like.py's EncoderLayerSANM; the forward is a SAN-M written from the public structure (embedding * sqrt(d) + pe, the
blocks with a residual each, after_norm, decoder), which the test also holds against tests/punc_ref.py in float32."""
import numpy as np
import torch
from torch import nn

import punc_ref as R
from funasr_like import EncoderLayerSANM, export_onnx


class _Encoder(nn.Module):
    def __init__(self, d, f, h, kernel, n_layers):
        super().__init__()
        self.encoders0 = nn.ModuleList([EncoderLayerSANM(d, d, f, h, kernel)])
        self.encoders = nn.ModuleList([EncoderLayerSANM(d, d, f, h, kernel) for _ in range(n_layers - 1)])
        self.after_norm = nn.LayerNorm(d)

    def forward(self, x):
        for layer in list(self.encoders0) + list(self.encoders):
            x = layer(x)
        return self.after_norm(x)


class CTTransformerLike(nn.Module):
    def __init__(self, vocab=64, d=256, f=1024, h=8, kernel=11, n_layers=2, n_punc=6, seed=0):
        super().__init__()
        torch.manual_seed(seed)
        self.embed = nn.Embedding(vocab, d)
        self.encoder = _Encoder(d, f, h, kernel, n_layers)
        self.decoder = nn.Linear(d, n_punc)
        self.scale = float(d) ** 0.5
        self.register_buffer("pe", torch.from_numpy(R.sinusoidal_pe(R.MAX_WINDOW, d)), persistent=False)
        with torch.no_grad():
            self.embed.weight.mul_(1.0 / 16.0)
            for m in self.modules():
                if isinstance(m, nn.LayerNorm):
                    m.weight.add_(0.05 * torch.randn_like(m.weight))
                    m.bias.add_(0.05 * torch.randn_like(m.bias))
                if isinstance(m, nn.Conv1d):
                    m.weight.mul_(0.3)

    def forward(self, text):
        """text int64 [B, T] -> logits [B, T, n_punc]"""
        x = self.embed(text) * self.scale + self.pe[: text.shape[1]]
        return self.decoder(self.encoder(x))


def export(module, T=9, opset=17) -> bytes:
    return export_onnx(module, (torch.zeros(1, T, dtype=torch.long),), ["text"], ["logits"], dynamic_axes=None, opset=opset)


def logits(module, ids) -> np.ndarray:
    with torch.no_grad():
        return module.eval()(torch.from_numpy(np.asarray(ids, dtype=np.int64))[None]).numpy()[0]
