"""An independent torch module with the parameter names of 3D-Speaker's CAMPPlus (as remembered: `head.*` the FCM, `xvector.*`
the D-TDNN) and a forward, for testing the converter (names, BatchNorm folding) and for holding against spk_ref (float32 against
float64).  Written from the architecture's description, not from 3D-Speaker's source."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F


def _nonlinear(channels, relu=True, affine=True):
    mods = [("batchnorm", nn.BatchNorm1d(channels, affine=affine))]
    if relu:
        mods.append(("relu", nn.ReLU()))
    return nn.Sequential(OrderedDict(mods))


class ResBlock(nn.Module):
    def __init__(self, m, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(m, m, 3, stride=(stride, 1), padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(m)
        self.conv2 = nn.Conv2d(m, m, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(m)
        self.shortcut = nn.Sequential()
        if stride != 1:
            self.shortcut = nn.Sequential(nn.Conv2d(m, m, 1, stride=(stride, 1), bias=False), nn.BatchNorm2d(m))

    def forward(self, x):
        y = F.relu(self.bn1(self.conv1(x)))
        return F.relu(self.bn2(self.conv2(y)) + self.shortcut(x))


class FCM(nn.Module):
    def __init__(self, m):
        super().__init__()
        self.conv1 = nn.Conv2d(1, m, 3, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(m)
        self.layer1 = nn.Sequential(ResBlock(m, 2), ResBlock(m, 1))
        self.layer2 = nn.Sequential(ResBlock(m, 2), ResBlock(m, 1))
        self.conv2 = nn.Conv2d(m, m, 3, stride=(2, 1), padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(m)

    def forward(self, x):                                  # [B, F, T]
        x = F.relu(self.bn1(self.conv1(x.unsqueeze(1))))
        x = self.layer2(self.layer1(x))
        x = F.relu(self.bn2(self.conv2(x)))
        return x.reshape(x.shape[0], x.shape[1] * x.shape[2], x.shape[3])


class CAMLayer(nn.Module):
    def __init__(self, bn, g, dilation, seg_len):
        super().__init__()
        self.linear_local = nn.Conv1d(bn, g, 3, dilation=dilation, padding=dilation, bias=False)
        self.linear1 = nn.Conv1d(bn, bn // 2, 1)
        self.linear2 = nn.Conv1d(bn // 2, g, 1)
        self.seg_len = seg_len

    def forward(self, x):
        y = self.linear_local(x)
        seg = F.avg_pool1d(x, self.seg_len, self.seg_len, ceil_mode=True)
        seg = seg.unsqueeze(-1).expand(*seg.shape, self.seg_len).reshape(*seg.shape[:-1], -1)[..., : x.shape[-1]]
        ctx = x.mean(-1, keepdim=True) + seg
        return y * torch.sigmoid(self.linear2(F.relu(self.linear1(ctx))))


class CAMDenseLayer(nn.Module):
    def __init__(self, C, bn, g, dilation, seg_len):
        super().__init__()
        self.nonlinear1 = _nonlinear(C)
        self.linear1 = nn.Conv1d(C, bn, 1, bias=False)
        self.nonlinear2 = _nonlinear(bn)
        self.cam_layer = CAMLayer(bn, g, dilation, seg_len)

    def forward(self, x):
        return self.cam_layer(self.nonlinear2(self.linear1(self.nonlinear1(x))))


class CAMDenseBlock(nn.ModuleList):
    def __init__(self, n, C, bn, g, dilation, seg_len):
        super().__init__()
        for i in range(n):
            self.add_module("tdnnd%d" % (i + 1), CAMDenseLayer(C + i * g, bn, g, dilation, seg_len))

    def forward(self, x):
        for layer in self:
            x = torch.cat([x, layer(x)], dim=1)
        return x


class Transit(nn.Module):
    def __init__(self, C):
        super().__init__()
        self.nonlinear = _nonlinear(C)
        self.linear = nn.Conv1d(C, C // 2, 1, bias=False)

    def forward(self, x):
        return self.linear(self.nonlinear(x))


class TDNN(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.linear = nn.Conv1d(cin, cout, 5, stride=2, padding=2, bias=False)
        self.nonlinear = _nonlinear(cout)

    def forward(self, x):
        return self.nonlinear(self.linear(x))


class Dense(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.linear = nn.Conv1d(cin, cout, 1, bias=False)
        self.nonlinear = _nonlinear(cout, relu=False, affine=False)

    def forward(self, x):
        return self.nonlinear(self.linear(x.unsqueeze(-1))).squeeze(-1)


class CAMPPlusLike(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        m, g, bn = int(cfg["m_channels"]), int(cfg["growth"]), int(cfg["bn_channels"])
        self.head = FCM(m)
        C = int(cfg["init_channels"])
        mods = [("tdnn", TDNN(m * (int(cfg["n_mels"]) // 8), C))]
        for i, (n, d) in enumerate(zip(cfg["blocks"], cfg["dilations"])):
            mods.append(("block%d" % (i + 1), CAMDenseBlock(int(n), C, bn, g, int(d), int(cfg["seg_len"]))))
            C += int(n) * g
            mods.append(("transit%d" % (i + 1), Transit(C)))
            C //= 2
        mods.append(("out_nonlinear", _nonlinear(C)))
        self.channels = C
        self.xvector = nn.Sequential(OrderedDict(mods))
        self.xvector.add_module("dense", Dense(2 * C, int(cfg["embedding"])))

    def frames(self, x):                                   # [B, T, F], already mean-normalised -> [B, C, T']
        y = self.head(x.permute(0, 2, 1))
        for name, mod in self.xvector.named_children():
            if name != "dense":
                y = mod(y)
        return y

    def forward(self, x):
        y = self.frames(x)
        stats = torch.cat([y.mean(-1), y.std(-1, unbiased=True)], dim=1)
        return self.xvector.dense(stats)


def random_module(cfg, seed, dtype=torch.float32):
    """the module in eval mode with seeded weights and BatchNorm statistics that are not the identity"""
    torch.manual_seed(seed)
    net = CAMPPlusLike(cfg)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for mod in net.modules():
            if isinstance(mod, (nn.BatchNorm1d, nn.BatchNorm2d)):
                mod.running_mean.copy_(0.2 * torch.randn(mod.num_features, generator=g))
                mod.running_var.copy_(0.5 + torch.rand(mod.num_features, generator=g))
                if mod.affine:
                    mod.weight.copy_(0.8 + 0.4 * torch.rand(mod.num_features, generator=g))
                    mod.bias.copy_(0.1 * torch.randn(mod.num_features, generator=g))
            elif isinstance(mod, (nn.Conv1d, nn.Conv2d)):
                fan = float(np.prod(mod.weight.shape[1:]))
                mod.weight.copy_(torch.randn(mod.weight.shape, generator=g) * (2.0 / fan) ** 0.5)
                if mod.bias is not None:
                    mod.bias.copy_(0.1 * torch.randn(mod.bias.shape, generator=g))
    return net.to(dtype).eval()


def embed(net, rows, dtype=torch.float32):
    """rows [T, n_mels] -> (frames [T', C], embedding [E]) as numpy, with the per-window mean subtracted first"""
    x = torch.as_tensor(np.asarray(rows, np.float32)).to(dtype)
    x = (x - x.mean(0, keepdim=True)).unsqueeze(0)
    with torch.no_grad():
        fr = net.frames(x)
        stats = torch.cat([fr.mean(-1), fr.std(-1, unbiased=True)], dim=1)
        emb = net.xvector.dense(stats)
    return fr[0].T.double().numpy(), emb[0].double().numpy()
