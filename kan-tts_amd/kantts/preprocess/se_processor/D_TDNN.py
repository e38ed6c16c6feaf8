"""DTDNN: the speaker-embedding extractor of SE voices -- a 2-D ResNet head over the 80 fbank bins, a strided TDNN, three
densely connected TDNN blocks (12 / 24 / 16 layers, dilation 1 / 2 / 3) with context-aware masking, statistics pooling and
a dense embedding layer.  State-dict names and shapes are those of a published ``se.model`` (``strict=True`` loads).

Two paths, eval mode only:
  * ``forward(feats)`` -- stock torch ops, any device, every item taken at the full width T (the yardstick);
  * ``forward(feats, lengths)`` on a HIP device, or ``forward_kernels`` -- the launches of csrc/spk_embed.hip over a ragged
    batch: every item is computed over its own frames only, so a batch gives each item its batch-1 result bit for bit."""
from collections import OrderedDict

import torch
import torch.nn.functional as F
from torch import nn

from .layers import DenseLayer, SEDenseTDNNBlock, StatsPool, TDNNLayer, TransitLayer, fold_bn

BLOCKS = ((12, 3, 1), (24, 3, 2), (16, 3, 3))  # (layers, kernel size, dilation) per dense block


class BasicBlock(nn.Module):
    """Two 3 x 3 convolutions over (F, T), the first with F-stride ``stride``, and a residual connection (a 1 x 1 strided
    shortcut when the shape changes)."""
    expansion = 1

    def __init__(self, in_planes, planes, stride=1):
        super().__init__()
        self.conv1 = nn.Conv2d(in_planes, planes, 3, stride=(stride, 1), padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=1, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.shortcut = nn.Sequential()
        self.stride = stride
        if stride != 1 or in_planes != planes:
            self.shortcut = nn.Sequential(nn.Conv2d(in_planes, planes, 1, stride=(stride, 1), bias=False),
                                          nn.BatchNorm2d(planes))

    def forward(self, x):
        out = F.relu(self.bn1(self.conv1(x)))
        return F.relu(self.bn2(self.conv2(out)) + self.shortcut(x))


class CNN_Head(nn.Module):
    """(B, F, T) -> (B, m_channels * F / 8, T): conv, two stages of two BasicBlocks and a conv, F halved three times."""

    def __init__(self, num_blocks=(2, 2), m_channels=32, feat_dim=80):
        super().__init__()
        self.conv1 = nn.Conv2d(1, m_channels, 3, stride=1, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(m_channels)
        self.layer1 = nn.Sequential(*[BasicBlock(m_channels, m_channels, s) for s in [2] + [1] * (num_blocks[0] - 1)])
        self.layer2 = nn.Sequential(*[BasicBlock(m_channels, m_channels, s) for s in [2] + [1] * (num_blocks[0] - 1)])
        self.conv2 = nn.Conv2d(m_channels, m_channels, 3, stride=(2, 1), padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(m_channels)
        self.out_channels = m_channels * (feat_dim // 8)

    def forward(self, x):
        out = F.relu(self.bn1(self.conv1(x.unsqueeze(1))))
        out = self.layer2(self.layer1(out))
        out = F.relu(self.bn2(self.conv2(out)))
        return out.reshape(out.shape[0], out.shape[1] * out.shape[2], out.shape[3])


class DTDNN(nn.Module):
    def __init__(self, feat_dim=80, embedding_size=192, growth_rate=32, bn_size=4, init_channels=128,
                 config_str="batchnorm-relu", memory_efficient=True):
        super().__init__()
        if config_str != "batchnorm-relu":
            raise NotImplementedError("DTDNN: only the batchnorm-relu configuration is carried, got %r" % (config_str,))
        self.feat_dim, self.embedding_size = feat_dim, embedding_size
        self.head = CNN_Head(feat_dim=feat_dim)
        self.xvector = nn.Sequential(OrderedDict([("tdnn", TDNNLayer(self.head.out_channels, init_channels, 5, stride=2))]))
        channels = init_channels
        for i, (num_layers, kernel_size, dilation) in enumerate(BLOCKS):
            self.xvector.add_module("block%d" % (i + 1), SEDenseTDNNBlock(num_layers, channels, growth_rate,
                                                                         bn_size * growth_rate, kernel_size, dilation))
            channels += num_layers * growth_rate
            self.xvector.add_module("transit%d" % (i + 1), TransitLayer(channels, channels // 2, bias=False))
            channels //= 2
        self.bn = nn.BatchNorm1d(channels)
        self.relu = nn.ReLU()
        self.xvector.add_module("stats", StatsPool())
        self.xvector.add_module("dense", DenseLayer(channels * 2, embedding_size))
        for m in self.modules():
            if isinstance(m, (nn.Conv1d, nn.Linear)):
                nn.init.kaiming_normal_(m.weight.data)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
        self._tables = {}
        self.eval()

    # -- weights ------------------------------------------------------------------------------------------------------
    def load_state_dict(self, *args, **kwargs):
        self._tables = {}
        return super().load_state_dict(*args, **kwargs)

    def _apply(self, fn, *args, **kwargs):
        self._tables = {}
        return super()._apply(fn, *args, **kwargs)

    def kernel_tables(self):
        """What the kernels read, built once per weight load: contiguous fp32 weights and every BatchNorm folded on the
        host (eval mode, running statistics) into (scale, shift)."""
        dev = self.bn.weight.device
        if dev not in self._tables:
            with torch.no_grad():
                self._tables[dev] = self._build_tables()
        return self._tables[dev]

    def _build_tables(self):
        def w(t):
            return t.detach().float().contiguous()

        h = self.head
        tb = {"conv1": (w(h.conv1.weight), fold_bn(h.bn1)), "conv2": (w(h.conv2.weight), fold_bn(h.bn2)), "blocks2d": []}
        for blk in list(h.layer1) + list(h.layer2):
            sc = None
            if len(blk.shortcut):
                sc = (w(blk.shortcut[0].weight).reshape(blk.shortcut[0].out_channels, -1).contiguous(),) + fold_bn(blk.shortcut[1])
            tb["blocks2d"].append(dict(stride=blk.stride, c1=(w(blk.conv1.weight), fold_bn(blk.bn1)),
                                       c2=(w(blk.conv2.weight), fold_bn(blk.bn2)), shortcut=sc))
        xv = self.xvector
        tb["tdnn"] = (w(xv.tdnn.linear.weight), fold_bn(xv.tdnn.nonlinear.batchnorm))
        tb["dense_blocks"] = []
        for i in range(len(BLOCKS)):
            block, transit = getattr(xv, "block%d" % (i + 1)), getattr(xv, "transit%d" % (i + 1))
            layers = []
            for layer in block:
                se = layer.se
                layers.append(dict(bn1=fold_bn(layer.nonlinear1.batchnorm), w1=w(layer.linear1.weight),
                                   bn2=fold_bn(layer.nonlinear2.batchnorm),
                                   wa=w(se.linear1.weight).reshape(se.linear1.out_channels, -1).contiguous(),
                                   ba=w(se.linear1.bias),
                                   wb=w(se.linear2.weight).reshape(se.linear2.out_channels, -1).contiguous(),
                                   bb=w(se.linear2.bias), w_stem=w(se.linear_stem.weight)))
            first = next(iter(block))
            tb["dense_blocks"].append(dict(layers=layers, dilation=block.dilation, c_in=first.linear1.in_channels,
                                           growth=first.se.linear_stem.out_channels,
                                           transit=(w(transit.linear.weight), fold_bn(transit.nonlinear.batchnorm))))
        tb["bn"] = fold_bn(self.bn)
        tb["dense"] = (w(xv.dense.linear.weight).reshape(self.embedding_size, -1).contiguous(),
                       fold_bn(xv.dense.nonlinear.batchnorm))
        return tb

    # -- forward ------------------------------------------------------------------------------------------------------
    def forward(self, feats, lengths=None):
        """feats (B, T, feat_dim) -> (B, embedding_size).  ``lengths`` (B): the items' own frame counts."""
        if self.training:
            raise NotImplementedError("DTDNN carries the inference graph only: call .eval() (training the speaker-embedding "
                                      "extractor is out of scope)")
        if lengths is None:
            return self._forward_stock(feats)
        if feats.is_cuda:
            return self.forward_kernels(feats, lengths)
        lens = [int(n) for n in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
        return torch.cat([self._forward_stock(feats[b:b + 1, :n]) for b, n in enumerate(lens)], dim=0)

    def _forward_stock(self, feats):
        xv = self.xvector
        x = xv.tdnn(self.head(feats.permute(0, 2, 1)))
        for i in range(len(BLOCKS)):
            x = getattr(xv, "transit%d" % (i + 1))(getattr(xv, "block%d" % (i + 1))(x))
        return xv.dense(xv.stats(self.relu(self.bn(x))))

    @torch.no_grad()
    def forward_kernels(self, feats, lengths):
        """The kernel path: 10 head launches, the TDNN, two launches per dense layer, a transit per block and the tail --
        119 launches for the shipped geometry whatever the batch.  ``lengths``: int32 device tensor (B), or a list (then
        no device value is read back to size the launches)."""
        from kantts._hip import ops

        if self.training:
            raise NotImplementedError("DTDNN carries the inference graph only: call .eval()")
        if feats.dim() != 3 or feats.shape[2] != self.feat_dim or feats.dtype != torch.float32:
            raise ValueError("DTDNN: feats must be fp32 (B, T, %d), got %s %s" % (self.feat_dim, feats.dtype, tuple(feats.shape)))
        B, T, _ = feats.shape
        if torch.is_tensor(lengths):
            lens, max_len = lengths.to(device=feats.device, dtype=torch.int32).contiguous(), int(lengths.max())
        else:
            max_len = max(int(n) for n in lengths)
            lens = torch.tensor([int(n) for n in lengths], dtype=torch.int32).to(feats.device)
        if max_len > T or int(lens.numel()) != B:
            raise ValueError("DTDNN: %d lengths (longest %d) for a batch of %d items of %d frames" % (lens.numel(), max_len, B, T))
        tb = self.kernel_tables()
        # head: (B, T, F) -> (B, 32, F, T) -> ... -> (B, 32 * F / 8, T)
        (w, (s, b)) = tb["conv1"]
        x = ops.spk_conv2d(feats, w, s, b, lens, feats_layout=True)
        for blk in tb["blocks2d"]:
            (w1, (s1, b1)), (w2, (s2, b2)) = blk["c1"], blk["c2"]
            mid = ops.spk_conv2d(x, w1, s1, b1, lens, sf=blk["stride"])
            x = ops.spk_conv2d(mid, w2, s2, b2, lens, res=x, shortcut=blk["shortcut"], rsf=blk["stride"])
        (w, (s, b)) = tb["conv2"]
        x = ops.spk_conv2d(x, w, s, b, lens, sf=2)
        x = x.view(B, x.shape[1] * x.shape[2], T)
        # TDNN (k = 5, stride 2) straight into the first block's buffer
        T2, max2 = (T - 1) // 2 + 1, (max_len - 1) // 2 + 1
        lens2 = torch.div(lens - 1, 2, rounding_mode="floor").to(torch.int32) + 1
        blocks = tb["dense_blocks"]
        work = ops.spk_cam_work(B, blocks[0]["layers"][0]["w1"].shape[0], T2, feats.device)

        def block_buffer(blk):
            return torch.empty((B, blk["c_in"] + len(blk["layers"]) * blk["growth"], T2), device=feats.device)

        buf = block_buffer(blocks[0])
        (w, post) = tb["tdnn"]
        ops.spk_conv1d(x, lens, w, buf, max2, post=post, stride=2)
        for i, blk in enumerate(blocks):
            for j, layer in enumerate(blk["layers"]):
                ops.spk_cam_layer(buf, lens2, blk["c_in"] + j * blk["growth"], layer, blk["dilation"], max2, work)
            (w, pre) = blk["transit"]
            nxt = block_buffer(blocks[i + 1]) if i + 1 < len(blocks) else torch.empty((B, w.shape[0], T2), device=feats.device)
            ops.spk_conv1d(buf, lens2, w, nxt, max2, pre=pre)
            buf = nxt
        (w, obn) = tb["dense"]
        return ops.spk_tail(buf, lens2, tb["bn"], w, obn)
