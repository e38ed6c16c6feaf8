"""Building blocks of the D-TDNN speaker-embedding extractor (inference graph only).

The module and parameter names are the ones a published ``se.model`` state dict carries, so it loads with
``strict=True``; what each block computes is written here in stock torch ops and is the yardstick the kernels of
csrc/spk_embed.hip are tested against.  Training the extractor is out of scope (DTDNN.forward refuses training mode)."""
import torch
import torch.nn.functional as F
from torch import nn

SEG_LEN = 100  # frames per segment of the context-aware mask's max pooling


def bn_relu(channels, affine=True, relu=True):
    """``batchnorm`` (+ ``relu``): the non-linearity every block of the graph uses, under the state-dict names."""
    seq = nn.Sequential()
    seq.add_module("batchnorm", nn.BatchNorm1d(channels, affine=affine))
    if relu:
        seq.add_module("relu", nn.ReLU())
    return seq


def fold_bn(bn):
    """Eval-mode BatchNorm as y = x * scale + shift (fp64 arithmetic, fp32 tables)."""
    var, mean = bn.running_var.double(), bn.running_mean.double()
    scale = 1.0 / torch.sqrt(var + bn.eps)
    if bn.affine:
        scale = scale * bn.weight.double()
    shift = -mean * scale
    if bn.affine:
        shift = shift + bn.bias.double()
    return scale.float().contiguous(), shift.float().contiguous()


class StatsPool(nn.Module):
    """(B, C, T) -> (B, 2 C): mean and unbiased standard deviation over time."""

    def forward(self, x):
        return torch.cat([x.mean(dim=-1), x.std(dim=-1, unbiased=True)], dim=-1)


class TDNNLayer(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, dilation=1):
        super().__init__()
        if kernel_size % 2 != 1:
            raise ValueError("TDNNLayer pads symmetrically: odd kernel sizes only, got %d" % kernel_size)
        self.linear = nn.Conv1d(in_channels, out_channels, kernel_size, stride=stride,
                                padding=(kernel_size - 1) // 2 * dilation, dilation=dilation, bias=False)
        self.nonlinear = bn_relu(out_channels)

    def forward(self, x):
        return self.nonlinear(self.linear(x))


class PoolingBlock(nn.Module):
    """Context-aware mask: the dilated stem convolution times a gate formed from the utterance mean plus the maximum of
    the frame's 100-frame segment (the last segment may be partial)."""

    def __init__(self, bn_channels, out_channels, kernel_size, dilation, reduction=2):
        super().__init__()
        self.linear_stem = nn.Conv1d(bn_channels, out_channels, kernel_size, padding=(kernel_size - 1) // 2 * dilation,
                                     dilation=dilation, bias=False)
        self.linear1 = nn.Conv1d(bn_channels, bn_channels // reduction, 1)
        self.relu = nn.ReLU()
        self.linear2 = nn.Conv1d(bn_channels // reduction, out_channels, 1)
        self.sigmoid = nn.Sigmoid()

    def gate(self, x):
        """(B, out_channels, T): the gate of every frame (constant inside a segment)."""
        T = x.shape[-1]
        seg = F.max_pool1d(x, kernel_size=SEG_LEN, stride=SEG_LEN, ceil_mode=True)
        ctx = x.mean(dim=-1, keepdim=True) + seg.repeat_interleave(SEG_LEN, dim=-1)[..., :T]
        return self.sigmoid(self.linear2(self.relu(self.linear1(ctx))))

    def forward(self, x):
        return self.linear_stem(x) * self.gate(x)


class SEDenseTDNNLayer(nn.Module):
    def __init__(self, in_channels, out_channels, bn_channels, kernel_size, dilation=1):
        super().__init__()
        self.nonlinear1 = bn_relu(in_channels)
        self.linear1 = nn.Conv1d(in_channels, bn_channels, 1, bias=False)
        self.nonlinear2 = bn_relu(bn_channels)
        self.se = PoolingBlock(bn_channels, out_channels, kernel_size, dilation)

    def forward(self, x):
        return self.se(self.nonlinear2(self.linear1(self.nonlinear1(x))))


class SEDenseTDNNBlock(nn.ModuleList):
    """``num_layers`` dense layers; layer i sees the block input and the outputs of the layers before it."""

    def __init__(self, num_layers, in_channels, out_channels, bn_channels, kernel_size, dilation=1):
        super().__init__()
        self.dilation = dilation
        for i in range(num_layers):
            self.add_module("tdnnd%d" % (i + 1), SEDenseTDNNLayer(in_channels + i * out_channels, out_channels, bn_channels,
                                                                  kernel_size, dilation))

    def forward(self, x):
        for layer in self:  # the stock path concatenates; the kernel path writes in place (ops.spk_cam_layer)
            x = torch.cat([x, layer(x)], dim=1)
        return x


class TransitLayer(nn.Module):
    def __init__(self, in_channels, out_channels, bias=True):
        super().__init__()
        self.nonlinear = bn_relu(in_channels)
        self.linear = nn.Conv1d(in_channels, out_channels, 1, bias=bias)

    def forward(self, x):
        return self.linear(self.nonlinear(x))


class DenseLayer(nn.Module):
    """1 x 1 dense layer on (B, C) or (B, C, T), followed by an affine-free BatchNorm."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.linear = nn.Conv1d(in_channels, out_channels, 1, bias=False)
        self.nonlinear = bn_relu(out_channels, affine=False, relu=False)

    def forward(self, x):
        if x.dim() == 2:
            return self.nonlinear(self.linear(x.unsqueeze(-1)).squeeze(-1))
        return self.nonlinear(self.linear(x))
