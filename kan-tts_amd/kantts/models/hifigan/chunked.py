"""Chunked HiFi-GAN inference with carried convolution state.

A causal ``Generator`` exists so that audio can be emitted while mel frames are still arriving (reference
kantts/models/hifigan/layers.py:52-165, hifigan.py:59-60); ``Generator.forward`` takes a whole utterance.
``ChunkedVocoder`` plays the same network chunk by chunk: every causal layer keeps the last ``H`` rows of its input
between calls (csrc/sconv.hip, kantts_sconv_launch), so the concatenated chunk outputs are the one-shot output up to
fp32 summation order.  A zero state is exactly the reference's zero left-pad, so a fresh slot needs no special case.

    v = ChunkedVocoder(generator, slots=S, graph=True)    # generator: causal, eval, on the device
    wav = v.step(mel)            # mel (S, C_mel, Tc), any Tc >= 1 -> wav (S, 1, Tc * prod(upsample_scales))
    v.reset(slot=None)           # one slot or all: the next step starts from zero state
    for wav in v.synthesize(mel_full, chunk_frames=8, slot=0): ...

The slots need not move in lockstep: ``step(mel, rows=counts)`` advances slot ``s`` by ``counts[s]`` frames only (0 holds
its state bit for bit; frames of ``mel`` past a slot's count are never read), through the per-slot row counts of
kantts_sconv_rows_launch.  ``play_many`` builds continuous batching on it:

    wav = v.step(mel, rows=[8, 3, 0, 8])                  # samples at and after rows[s] * hop of slot s are 0.0
    for index, wav in v.play_many(mels, chunk_frames=8): ...   # utterances of any lengths through all slots

``synthesize`` and ``play_many`` are defined here once, for this class and its four subclasses (chunked_nsf, chunked_mb,
chunked_nc, chunked_nc_nsf): one schedule (``schedule``) on three per-class facts, the emission contract in the hook block
of the class.  kantts.models.streaming.StreamingTTS is written on the same three facts.

History rows per layer (at that layer's token rate): ``(k - 1) * dilation`` for a convolution, ``J - 1`` input tokens
for an upsampling stage (J polyphase taps: the transposed convolution alone has kernel / stride, the fused dual-path
stage of ``Generator._dual_path_weight`` max(kernel / stride, 1 + ceil(6 / stride))).
"""
import operator

import torch

import kantts._hip as hip
from kantts._hip import ops
from kantts.models.hifigan.layers import CausalConv1d, CausalConvTranspose1d, effective_weight

# what kantts_sconv_launch accepts (include/kantts_hip.h); checked here BEFORE anything is packed or launched
_MAX_K, _MAX_STEP = 11, 7


def sconv_supported(Cin, N, K, step):
    return (Cin % 8 == 0 and 16 <= Cin <= 512 and (N == 1 or 16 <= N <= 4096) and 1 <= K <= _MAX_K
            and 1 <= step <= _MAX_STEP)


def slot_ints(vals, what, slots, bools=False):
    """One integer per slot -- a sequence of ints, or an integer tensor of shape (slots,) on the host or on the device --
    as a host list, or None for a device tensor (it is not read back).  The one check of ``rows``, ``end`` and ``last``;
    what differs between the three is applied by the caller, on purpose:

    rows   a count: host values must lie in [0, Tc] (a ValueError), device values are clamped by the kernel.  Bool tensors
           are refused (``bools``) -- except that ``ChunkedMBVocoder.step`` takes a HOST bool tensor, which it hands on as
           a list of 0 / 1 (a device one reaches the base class and is refused there): it always did
    end    a frame count: values of a sequence below -1 become -1 ("open"); a tensor, on the host or on the device, is
           copied as it is (the kernel reads any negative value as open).  Bool tensors are refused
    last   a flag: host values become 0 / 1, device values are copied as they are (the kernel tests for non-zero); bool
           tensors are accepted"""
    if torch.is_tensor(vals):
        if vals.dtype.is_floating_point or vals.dtype.is_complex or (vals.dtype == torch.bool and not bools):
            raise ValueError("%s must be integers, got dtype %s" % (what, vals.dtype))
        if tuple(vals.shape) != (slots,):
            raise ValueError("%s must have shape (%d,), got %s" % (what, slots, tuple(vals.shape)))
        if vals.device.type != "cpu":
            return None
        vals = vals.tolist()
    try:
        vals = [operator.index(v) for v in vals]
    except TypeError:
        raise ValueError("%s must be a sequence of %d ints or an integer tensor" % (what, slots)) from None
    if len(vals) != slots:
        raise ValueError("%s must hold one integer per slot (%d), got %d" % (what, slots, len(vals)))
    return vals


def schedule(lengths, slots, chunk_frames, flush_frames=0):
    """The one schedule of continuous batching, on host integers alone: utterances of ``lengths`` frames through ``slots``
    slots that take up to ``chunk_frames`` frames per step.  A free slot takes the next unassigned utterance, in input
    order and slot order, before a step; a slot at ``pos`` of an utterance of T frames takes
    min(chunk_frames, T + flush_frames - pos) frames, of which max(0, min(take, T - pos)) are live (the others are flush
    frames behind the utterance's end), and is free again once pos >= T + flush_frames.  Yields, per step, one entry per
    slot: None for an idle slot, else ``(index, pos, take, live, done)`` with ``pos`` the frames consumed BEFORE the step
    (0: the slot has just taken the utterance) and ``done`` true when the slot is free after it."""
    cur, pos, nxt = [None] * slots, [0] * slots, 0
    while True:
        for s in range(slots):
            if cur[s] is None and nxt < len(lengths):
                cur[s], pos[s], nxt = nxt, 0, nxt + 1
        if all(c is None for c in cur):
            return
        plan = [None] * slots
        for s, c in enumerate(cur):
            if c is not None:
                take = min(chunk_frames, lengths[c] + flush_frames - pos[s])
                plan[s] = (c, pos[s], take, max(0, min(take, lengths[c] - pos[s])),
                           pos[s] + take >= lengths[c] + flush_frames)
        yield plan
        for s, p in enumerate(plan):
            if p is not None:
                pos[s] += p[2]
                if p[4]:
                    cur[s] = None


class _Layer:
    """One stateful layer: geometry first (``plan``), packed weights later (``pack``)."""

    def __init__(self, name, Cin, N, K, step, in_leaky):
        self.name, self.Cin, self.N, self.K, self.step, self.in_leaky = name, Cin, N, K, step, in_leaky
        self.H = (K - 1) * step
        self.off = 0  # first float of this layer's state inside a slot of the arena
        self.w = self.bias = None


class ChunkedVocoder:
    """Chunk-by-chunk inference of a causal single-band ``Generator`` on ``slots`` independent utterances that advance
    by ``Tc`` frames per ``step`` -- together, or each by its own count of at most ``Tc`` (``step(mel, rows=...)``).

    The object is a SNAPSHOT of the generator: the effective (weight-normed, dual-path-fused) weights are computed and
    packed once, here; build a new ``ChunkedVocoder`` after the generator's weights change.  The contraction mode is
    ``kantts._hip.get_precision()`` at construction.

    All state of all layers lives in one arena ``(2, slots, L)`` fp32 (ping and pong halves, slot-major); its size depends
    on the model and ``slots`` only, so consecutive steps may use different chunk sizes.  A step reads half ``p`` and writes
    half ``1 - p`` inside the convolution launches themselves.

    ``graph=True``: a step is captured per distinct ``Tc`` -- one ``torch.cuda.CUDAGraph`` for each parity, on one stream
    with no parallel branches -- and replayed; ``mel`` is copied into a static buffer.  ``graph=False`` issues the same
    launches eagerly and gives identical bits.  The ``rows`` form of a step has graphs of its own (also per ``Tc``): the
    counts live in one int32 device buffer that the captured launches read, so they change between replays without a
    new capture (``captures`` counts the captures of the object).

    Refused at construction: non-causal generators (kantts.models.hifigan.chunked_nc.ChunkedNCVocoder plays them, late by
    the network's look-ahead), NSF generators (the excitation's running phase and random draws need
    a carried state of their own: kantts.models.hifigan.chunked_nsf.ChunkedNSFVocoder plays them), ``out_channels > 1``
    (the PQMF synthesis looks ahead: kantts.models.hifigan.chunked_mb.ChunkedMBVocoder plays them), and channel counts / kernel sizes the kernel declines (Cin a multiple of 8 in 16..512, k <= 11,
    dilation <= 7, upsampling N = scale * Cout <= 4096)."""

    _plays_nsf = False  # kantts.models.hifigan.chunked_nsf.ChunkedNSFVocoder carries the excitation's state
    _plays_multiband = False  # kantts.models.hifigan.chunked_mb.ChunkedMBVocoder runs conv_post inside the multi-band tail
    _plays_noncausal = False  # kantts.models.hifigan.chunked_nc.ChunkedNCVocoder delays, windows and flushes
    _conv_cls, _up_cls = CausalConv1d, CausalConvTranspose1d  # what the layers of the generator must be

    def __init__(self, generator, slots=1, graph=True, max_graphs=8):
        g = generator
        if not getattr(g, "causal", False) and not self._plays_noncausal:
            raise ValueError("ChunkedVocoder needs a causal generator (causal=True): a symmetric convolution looks ahead")
        if g.nsf_enable and not self._plays_nsf:
            raise NotImplementedError("ChunkedVocoder: NSF generators are not supported (the source module's running phase "
                                      "and random draws need a carried state of their own)")
        if g.out_channels != 1 and not self._plays_multiband:
            raise NotImplementedError("ChunkedVocoder: out_channels > 1 (multi-band / PQMF) generators are not supported")
        if g.training:
            raise ValueError("ChunkedVocoder needs generator.eval()")
        if int(slots) < 1:
            raise ValueError("slots must be >= 1")
        mode = hip.get_precision()
        if mode not in ("fp32", "bf16"):
            raise ValueError("ChunkedVocoder: precision %r has no chunked kernels" % mode)
        self.precision = hip.PREC_BF16 if mode == "bf16" else hip.PREC_FP32
        self.slots = int(slots)
        self.slope = g.slope
        self.scales = [int(s) for s in g.upsample_scales]
        self.hop = 1
        for s in self.scales:
            self.hop *= s
        self.num_kernels = g.num_kernels

        # ---- geometry of every stateful layer, from the modules' shapes alone (nothing is computed or launched yet)
        def conv_layer(name, m, in_leaky):
            if not isinstance(m, self._conv_cls) or m.causal == self._plays_noncausal:
                raise ValueError("ChunkedVocoder: %s is not a %s" % (name, self._conv_cls.__name__))
            c = m.conv1d
            if c.stride[0] != 1 or c.groups != 1:
                raise NotImplementedError("ChunkedVocoder: %s has stride / groups != 1" % name)
            return _Layer(name, c.in_channels, c.out_channels, c.kernel_size[0], c.dilation[0], in_leaky)

        self.in_channels = g.conv_pre.conv1d.in_channels
        self.pre = conv_layer("conv_pre", g.conv_pre, None)
        self.stages = []
        for i, s in enumerate(self.scales):
            up = g.transpose_upsamples[i][1]
            if not isinstance(up, self._up_cls):
                raise ValueError("ChunkedVocoder: transpose_upsamples[%d] is not %s" % (
                    i, "causal" if self._up_cls is CausalConvTranspose1d else "a " + self._up_cls.__name__))
            d = up.deconv
            J = self._stage_taps(g, i, s)
            upl = _Layer("stage%d.up" % i, d.in_channels, s * d.out_channels, J, 1, self.slope)
            stacks = []
            for j, blk in enumerate(g.conv_blocks[i * g.num_kernels:(i + 1) * g.num_kernels]):
                pairs = []
                for n, (c1, c2) in enumerate(zip(blk.convs1, blk.convs2)):
                    if blk.slope != self.slope:
                        raise NotImplementedError("ChunkedVocoder: residual blocks with their own activation slope")
                    pairs.append((conv_layer("stage%d.block%d.convs1.%d" % (i, j, n), c1, self.slope),
                                  conv_layer("stage%d.block%d.convs2.%d" % (i, j, n), c2, self.slope)))
                stacks.append(pairs)
            self.stages.append((s, d.out_channels, upl, stacks))
        self.post = conv_layer("conv_post", g.conv_post, 0.01)  # F.leaky_relu's default slope (reference hifigan.py:178)
        self.layers = [self.pre]
        for _, _, upl, stacks in self.stages:
            self.layers.append(upl)
            for pairs in stacks:
                for c1, c2 in pairs:
                    self.layers += [c1, c2]
        self.layers.append(self.post)
        for L in self.layers:
            if L is self.post and self._plays_multiband:
                continue  # checked by the subclass against the contract of its own kernel (_plan_extra)
            if not sconv_supported(L.Cin, L.N, L.K, L.step):
                raise NotImplementedError(
                    "ChunkedVocoder: layer %s (Cin %d, N %d, k %d, dilation %d) is outside what kantts_sconv_launch accepts "
                    "(Cin a multiple of 8 in 16..512, N = 1 or 16..4096, k <= %d, dilation <= %d)"
                    % (L.name, L.Cin, L.N, L.K, L.step, _MAX_K, _MAX_STEP))
        off = 0
        for L in self.layers:
            L.off = off
            off += L.H * L.Cin  # Cin % 8 == 0: every layer's state starts on a 16-byte boundary
        self.state_floats = off
        self._step_channels = self.in_channels  # channels of what ``step`` takes
        self._plan_extra(g)

        # ---- snapshot of the weights
        self.device = next(g.parameters()).device
        if graph and self.device.type != "cuda":
            raise ValueError("graph=True needs the generator on the GPU")
        self.graph = bool(graph)
        wdt = torch.bfloat16 if self.precision == hip.PREC_BF16 else torch.float32

        def pack(L, w_knc, bias):
            assert tuple(w_knc.shape) == (L.K, L.N, L.Cin), (L.name, tuple(w_knc.shape), (L.K, L.N, L.Cin))
            fp32 = L.N == 1 or (L is self.post and self._plays_multiband)  # the last layer is fp32 in both modes
            L.w = w_knc.detach().to(torch.float32 if fp32 else wdt).contiguous().clone()
            L.bias = None if bias is None else bias.detach().float().contiguous().clone()

        def pack_conv(L, m):
            w = effective_weight(m.conv1d)  # (Cout, Cin, k); tap j of the kernel reads j * dilation rows back = W[.., k-1-j]
            pack(L, w.permute(2, 0, 1).flip(0), m.conv1d.bias)

        with torch.no_grad():
            pack_conv(self.pre, g.conv_pre)
            for i, (s, Cout, upl, stacks) in enumerate(self.stages):
                w, b = self._stage_weight(g, i, s)  # (Cin, Cout, J*s)
                w2 = w.reshape(upl.Cin, Cout, upl.K, s).permute(2, 3, 1, 0).reshape(upl.K, s * Cout, upl.Cin)
                pack(upl, w2, None if b is None else b.repeat(s))
                blocks = g.conv_blocks[i * g.num_kernels:(i + 1) * g.num_kernels]
                for pairs, blk in zip(stacks, blocks):
                    for (l1, l2), c1, c2 in zip(pairs, blk.convs1, blk.convs2):
                        pack_conv(l1, c1)
                        pack_conv(l2, c2)
            pack_conv(self.post, g.conv_post)
        self.arena = torch.zeros(2, self.slots, max(self.state_floats, 4), device=self.device, dtype=torch.float32)
        self._rows = torch.zeros(self.slots, device=self.device, dtype=torch.int32)  # per-slot counts of step(rows=...)
        self._parity = 0
        self._graphs = {}
        self._max_graphs = int(max_graphs)
        self.captures = 0

    # ------------------------------------------------------------------------------------------------------------
    # the polyphase form of an upsampling stage (ChunkedNCVocoder has the symmetric stage's)
    def _stage_taps(self, g, i, s):
        """J: input tokens per output row of stage ``i`` (stride ``s``), from shapes alone."""
        d = g.transpose_upsamples[i][1].deconv
        if d.kernel_size[0] % s:
            raise NotImplementedError("ChunkedVocoder: upsampling kernel %d is not a multiple of its stride %d"
                                      % (d.kernel_size[0], s))
        J = d.kernel_size[0] // s
        if g.repeat_upsample:
            k7 = g.repeat_upsamples[i][2].conv1d.kernel_size[0]
            J = max(J, 1 + -(-(k7 - 1) // s))
        return J

    def _stage_weight(self, g, i, s):
        """(Cin, Cout, J * s) weight and (Cout) bias of stage ``i`` as one causal transposed convolution."""
        if g.repeat_upsample:
            return g._dual_path_weight(i, s)
        d = g.transpose_upsamples[i][1].deconv
        return effective_weight(d), d.bias

    # ------------------------------------------------------------------------------------------------------------
    # hooks of the subclasses; here they do nothing and the launches of a step are the ones of _run alone
    def _plan_extra(self, g):
        """Further refusals, decided from shapes before anything is packed."""

    def _assign(self, slot, index):
        """``play_many``: ``slot`` (just reset) takes utterance ``index``."""

    # The emission contract: three facts per class, on host integers alone.  ``pos``: frames the slot's vocoder has
    # consumed since its reset, ``n``: the frames it takes now, ``T``: the frames of its utterance.  ``play_many``,
    # ``synthesize`` and kantts.models.streaming.StreamingTTS are written on them and on nothing else of a subclass.
    flush_frames = 0  # 1. frames a slot must take behind its utterance's last one
    _end_kw = None    # 2. the keyword through which ``step`` is told an utterance's end (None: it is not told), and

    def _end_of(self, pos, n, T):
        """the slot's integer under that keyword; an idle slot asks with (0, 0, -1)."""

    def _emitted(self, pos, n, T):
        """3. (offset, count) of the slot's samples inside the step's output."""
        return 0, n * self.hop

    _solo = False  # ``synthesize`` advances its slot alone, through the ``rows`` form of a step (``_play_one``)

    def _solo_end(self, slot, pos, n, T):
        """The keyword arguments that tell a step of ``_play_one`` the end of ``slot`` alone: the others are idle."""
        if self._end_kw is None:
            return {}
        ends = [self._end_of(0, 0, -1)] * self.slots
        ends[slot] = self._end_of(pos, n, T)
        return {self._end_kw: ends}

    def _save_state(self):
        return self.arena.clone()

    def _restore_state(self, saved):
        self.arena.copy_(saved)

    def reset(self, slot=None):
        """Zero state for one slot (others untouched) or for all: one fill launch."""
        if slot is None:
            self.arena.zero_()
        else:
            if not 0 <= int(slot) < self.slots:
                raise IndexError("slot %r of %d" % (slot, self.slots))
            self.arena[:, int(slot)].zero_()

    def _conv(self, L, x, parity, res=None, rows=None, row_mul=1, zero_tail=False):
        S, T, _ = x.shape
        out = torch.empty((S, T, L.N), device=x.device, dtype=torch.float32)
        hin = hout = None
        if L.H:
            hin = self.arena[parity, 0, L.off:L.off + L.H * L.Cin]
            hout = self.arena[1 - parity, 0, L.off:L.off + L.H * L.Cin]
        ok = hip.sconv(x, hin, hout, L.w, out, S=S, Tc=T, Cin=L.Cin, N=L.N, K=L.K, step=L.step,
                       hist_ss=self.arena.shape[2], precision=self.precision, bias=L.bias, res=res, in_leaky=L.in_leaky,
                       **({} if rows is None else dict(rows=rows, row_mul=row_mul, zero_tail=zero_tail)))
        if not ok:
            raise RuntimeError("kantts_sconv_launch declined layer %s it was planned for" % L.name)
        return out

    def _run(self, mel, parity, rows=None, stage_res=None):
        """The launches of one step: mel (S, C, Tc) fp32 -> wav (S, 1, Tc * hop).  Reads arena[parity], writes
        arena[1 - parity].  ``rows``: the int32 device buffer of per-slot frame counts (every layer passes its own rows
        per frame; the element-wise launches run over the whole buffers -- what they do to dead rows is never read).
        ``stage_res``: one (S, rows, Cout) tensor per stage, added by the stage's up-layer launch (the NSF excitation)."""
        with torch.no_grad():
            mul = 1  # rows of the current layer per mel frame
            h = self._conv(self.pre, mel.transpose(1, 2).contiguous(), parity, rows=rows, row_mul=mul)
            for i, (s, Cout, upl, stacks) in enumerate(self.stages):
                h = ops.sin_add(h)
                res = None if stage_res is None else stage_res[i]
                h = self._conv(upl, h, parity, res=res, rows=rows, row_mul=mul).view(h.shape[0], h.shape[1] * s, Cout)
                mul *= s
                ys = []
                for pairs in stacks:  # sequential, as Generator._residual_stacks runs them under no_grad
                    x = h
                    for c1, c2 in pairs:
                        x = self._conv(c2, self._conv(c1, x, parity, rows=rows, row_mul=mul), parity, res=x, rows=rows,
                                       row_mul=mul)
                    ys.append(x)
                h = ops.mean_many(ys) if len(ys) > 1 else ys[0]
            return self._tail(h, parity, rows, mul)

    def _tail(self, h, parity, rows, mul):
        """The last launches of a step: h (S, Tc * prod(scales), C) -> wav (S, 1, samples)."""
        h = self._conv(self.post, h, parity, rows=rows, row_mul=mul, zero_tail=True)  # tanh(0) == 0: a silent tail
        return torch.tanh(h).transpose(1, 2)

    def _captured(self, Tc, with_rows=False):
        key = ("rows", Tc) if with_rows else Tc
        rows = self._rows if with_rows else None
        ent = self._graphs.pop(key, None)
        if ent is None:
            if len(self._graphs) >= self._max_graphs:
                self._graphs.pop(next(iter(self._graphs)))  # least recently used
            mel = torch.zeros(self.slots, self._step_channels, Tc, device=self.device, dtype=torch.float32)
            # eager warm-up of both parities on a side stream (kernels loaded, allocator primed); the state it advances
            # is put back afterwards
            saved = self._save_state()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for p in (0, 1):
                    self._run(mel, p, rows)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graphs, outs = [], []
            for p in (0, 1):
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr, capture_error_mode="thread_local"):
                    outs.append(self._run(mel, p, rows))
                graphs.append(gr)
            self._restore_state(saved)
            self.captures += 1
            ent = (mel, graphs, outs)
        self._graphs[key] = ent
        return ent

    def _set_rows(self, rows, Tc):
        """Validate per-slot counts and copy them into the persistent device buffer the launches read."""
        vals = slot_ints(rows, "rows", self.slots)
        if vals is None:  # on the device, not read back: the kernel clamps what it finds
            self._rows.copy_(rows)
            return
        if any(r < 0 or r > Tc for r in vals):
            raise ValueError("rows must lie in [0, Tc = %d], got %s" % (Tc, vals))
        self._rows.copy_(torch.tensor(vals, dtype=torch.int32))

    def step(self, mel, rows=None):
        """mel (slots, C_mel, Tc), Tc >= 1 -> wav (slots, 1, Tc * prod(upsample_scales)); advances every slot by Tc.

        ``rows``: ``slots`` ints in [0, Tc] (a sequence, or an integer tensor of shape (slots,) on the host or on the
        device; device values are clamped by the kernel, not read back).  Slot ``s`` advances by ``rows[s]`` frames: frames
        of ``mel`` at and after ``rows[s]`` are not read (they may hold anything), samples of ``wav`` at and after
        ``rows[s] * hop`` are 0.0, and a slot with ``rows[s] == 0`` keeps its state bit for bit."""
        if mel.dim() != 3 or mel.shape[0] != self.slots or mel.shape[1] != self._step_channels or mel.shape[2] < 1:
            raise ValueError("mel must be (slots=%d, %d, Tc >= 1), got %s" % (self.slots, self._step_channels, tuple(mel.shape)))
        Tc = int(mel.shape[2])
        if rows is not None:
            self._set_rows(rows, Tc)
        if self.graph:
            buf, graphs, outs = self._captured(Tc, rows is not None)
            buf.copy_(mel)
            graphs[self._parity].replay()
            wav = outs[self._parity].clone()
        else:
            wav = self._run(mel.to(device=self.device, dtype=torch.float32), self._parity,
                            None if rows is None else self._rows)
        self._parity ^= 1
        return wav

    def synthesize(self, mel_full, chunk_frames=8, slot=0, **identity):
        """Generator over the chunks of one utterance: mel_full (C, T) or (1, C, T), C what ``step`` takes, played on
        ``slot`` from zero state; ``identity`` goes to ``reset`` (the NSF classes: ``key=``).  A causal single-band class
        feeds the other slots zeros and they advance with it; every other class advances ``slot`` alone (``_play_one``).
        The last partial chunk is padded with zero frames and its output trimmed; ``flush_frames`` frames follow the
        utterance's last one.  Yields the (1, n_samples) tensors of the chunks that emit samples, T * hop in all."""
        if mel_full.dim() == 3:
            mel_full = mel_full[0]
        T = int(mel_full.shape[1])
        n = int(chunk_frames)
        if n < 1:
            raise ValueError("chunk_frames must be >= 1")
        self.reset(slot, **identity)
        yield from self._play_one(mel_full, T, n, slot)

    def _play_one(self, mel_full, T, n, slot):
        """The steps of ``synthesize`` on a slot that has just been reset."""
        if not self._solo:
            # The causal single-band classes keep the plain lockstep step ON PURPOSE: every slot advances (the others on
            # zero frames), and the plain step has a graph key of its own, so what ``synthesize`` leaves in the other
            # slots and in ``captures`` is observable and stays what it was.
            for t0 in range(0, T, n):
                t1 = min(T, t0 + n)
                mel = torch.zeros(self.slots, self._step_channels, n, device=self.device, dtype=torch.float32)
                mel[slot, :, :t1 - t0] = mel_full[:, t0:t1]
                yield self.step(mel)[slot, :, :(t1 - t0) * self.hop]
            return
        for plan in schedule([T] if T + self.flush_frames else [], 1, n, self.flush_frames):  # nothing to take: no steps
            _, pos, take, live, _ = plan[0]
            mel = torch.zeros(self.slots, self._step_channels, n, device=self.device, dtype=torch.float32)
            mel[slot, :, :live] = mel_full[:, pos:pos + live]
            rows = [0] * self.slots
            rows[slot] = take
            wav = self.step(mel, rows=rows, **self._solo_end(slot, pos, take, T))
            off, cnt = self._emitted(pos, take, T)
            if cnt:
                yield wav[slot, :, off:off + cnt]

    def play_many(self, mels, chunk_frames=8):
        """Continuous batching, for every class: a generator that plays the utterances ``mels`` -- a sequence of (C, T_i)
        tensors, T_i >= 1 -- through all slots, yielding ``(index, wav)`` with wav (1, samples) what utterance ``index``
        emitted in a step (a causal single-band class: n * hop for the ``n`` frames it advanced by; steps in which it
        emitted nothing yield nothing).  ``reset()`` once, then the steps of ``schedule``: the slots that have just taken
        an utterance are named it (``_assign``) in slot order; one ``step`` with every slot's count and end; the slots
        yield in slot order; a slot whose utterance is through (``flush_frames`` included) is ``reset(slot)``.  The
        concatenated chunks of an utterance equal ``synthesize`` of it bit for bit."""
        n = int(chunk_frames)
        if n < 1:
            raise ValueError("chunk_frames must be >= 1")
        mels = list(mels)
        for i, m in enumerate(mels):
            if m.dim() != 2 or m.shape[0] != self._step_channels or m.shape[1] < 1:
                raise ValueError("mels[%d] must be (%d, T >= 1), got %s" % (i, self._step_channels, tuple(m.shape)))
        lengths = [int(m.shape[1]) for m in mels]
        self.reset()
        buf = torch.zeros(self.slots, self._step_channels, n, device=self.device, dtype=torch.float32)
        for plan in schedule(lengths, self.slots, n, self.flush_frames):
            rows, ends = [0] * self.slots, [self._end_of(0, 0, -1)] * self.slots
            for s, p in enumerate(plan):
                if p is not None:
                    c, pos, take, live, _ = p
                    if pos == 0:
                        self._assign(s, c)
                    rows[s], ends[s] = take, self._end_of(pos, take, lengths[c])
                    buf[s, :, :live] = mels[c][:, pos:pos + live]
            wav = self.step(buf, rows=rows, **({} if self._end_kw is None else {self._end_kw: ends}))
            for s, p in enumerate(plan):
                if p is not None:
                    off, cnt = self._emitted(p[1], p[2], lengths[p[0]])
                    if cnt:
                        yield p[0], wav[s, :, off:off + cnt]
            for s, p in enumerate(plan):
                if p is not None and p[4]:
                    self.reset(s)
