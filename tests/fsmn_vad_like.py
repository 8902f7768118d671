"""A torch module with the parameter names and the arithmetic of FunASR's FSMN-VAD encoder
(funasr/models/fsmn_vad_streaming/encoder.py: FSMN under `encoder.`), restated from the public sources for the converter
tests: AffineTransform / LinearTransform wrap an nn.Linear as `.linear`, FSMNBlock holds the depthwise `conv_left`
(Conv2d [proj, 1, lorder, 1], dilation lstride), BasicBlock is linear -> fsmn_block -> affine -> ReLU.  The export form takes
and returns the per-block caches and ends in a Softmax, as FunASR's export does."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from funasr_like import export_onnx


class _Wrap(nn.Module):
    def __init__(self, n_in, n_out, bias):
        super().__init__()
        self.linear = nn.Linear(n_in, n_out, bias=bias)

    def forward(self, x):
        return self.linear(x)


class FSMNBlock(nn.Module):
    def __init__(self, dim, lorder, lstride):
        super().__init__()
        self.lorder, self.lstride = lorder, lstride
        self.conv_left = nn.Conv2d(dim, dim, [lorder, 1], dilation=[lstride, 1], groups=dim, bias=False)

    def forward(self, x, cache):
        x_per = x.unsqueeze(1).permute(0, 3, 2, 1)                     # [B, D, T, 1]
        y_left = torch.cat((cache, x_per), dim=2)                      # cache [B, D, (lorder - 1) * lstride, 1]
        new_cache = y_left[:, :, -(self.lorder - 1) * self.lstride:, :]
        out = x_per + self.conv_left(y_left)
        return out.permute(0, 3, 2, 1).squeeze(1), new_cache


class BasicBlock(nn.Module):
    def __init__(self, linear_dim, proj_dim, lorder, lstride):
        super().__init__()
        self.linear = _Wrap(linear_dim, proj_dim, False)
        self.fsmn_block = FSMNBlock(proj_dim, lorder, lstride)
        self.affine = _Wrap(proj_dim, linear_dim, True)

    def forward(self, x, cache):
        y, c = self.fsmn_block(self.linear(x), cache)
        return F.relu(self.affine(y)), c


class FSMN(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.in_linear1 = _Wrap(cfg["input_dim"], cfg["affine_dim"], True)
        self.in_linear2 = _Wrap(cfg["affine_dim"], cfg["linear_dim"], True)
        self.fsmn = nn.ModuleList([BasicBlock(cfg["linear_dim"], cfg["proj_dim"], cfg["lorder"], cfg["lstride"])
                                   for _ in range(cfg["n_layers"])])
        self.out_linear1 = _Wrap(cfg["linear_dim"], cfg["affine_dim"], True)
        self.out_linear2 = _Wrap(cfg["affine_dim"], cfg["output_dim"], True)

    def forward(self, x, caches):
        x = F.relu(self.in_linear2(self.in_linear1(x)))
        out = []
        for blk, c in zip(self.fsmn, caches):
            x, c = blk(x, c)
            out.append(c)
        return self.out_linear2(self.out_linear1(x)), out


class FsmnVadLike(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = dict(cfg)
        self.encoder = FSMN(cfg)

    def caches(self, B=1):
        c = self.cfg
        return [torch.zeros(B, c["proj_dim"], (c["lorder"] - 1) * c["lstride"], 1) for _ in range(c["n_layers"])]

    def forward(self, speech, *caches):
        z, out = self.encoder(speech, list(caches))
        return (torch.softmax(z, dim=-1), *out)

    def logits(self, speech):
        return self.encoder(speech, self.caches(speech.shape[0]))[0]


def load_pfw_weights(module, cfg, w):
    """PFW "fsmnvad" tensors -> the module's parameters through convert.vad_name_map"""
    from aliparaformerasr_amd import convert as cv
    sd = module.state_dict()
    for pk, fk in cv.vad_name_map(cfg["n_layers"]).items():
        a = np.asarray(w[pk], np.float32)
        if pk.endswith(".taps"):
            a = a.T[:, None, :, None]                                   # [lorder, proj] -> [proj, 1, lorder, 1]
        assert tuple(sd[fk].shape) == a.shape, (fk, tuple(sd[fk].shape), a.shape)
        sd[fk] = torch.from_numpy(np.ascontiguousarray(a))
    module.load_state_dict(sd)


def export(module, T=7, opset=17) -> bytes:
    n = module.cfg["n_layers"]
    names_in = ["speech"] + ["in_cache%d" % i for i in range(n)]
    names_out = ["logits"] + ["out_cache%d" % i for i in range(n)]
    args = (torch.zeros(1, T, module.cfg["input_dim"]), *module.caches())
    return export_onnx(module, args, names_in, names_out, dynamic_axes={"speech": {1: "T"}, "logits": {1: "T"}}, opset=opset)
