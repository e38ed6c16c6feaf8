"""Chunked inference for NON-CAUSAL HiFi-GAN generators (single band, no source module).

A symmetric network is a causal network whose tensors are delayed, whose zero padding is applied at the utterance's edges
rather than the chunk's, and whose end is flushed.  Every tensor gets an integer delay ``d`` in rows at its own rate: row n
of its stream, counted from the slot's reset, is true row n - d of the utterance (the mel input has d = 0).

    symmetric convolution (k, dilation, padding p = (k - 1) dilation / 2)   the causal layer with the same taps, d_out = d_in + p
    residual pair x + c2(c1(x))            d_out = d_in + p1 + p2; the residual is x read p1 + p2 rows back, through the
                                           state c1 keeps anyway (p2 <= p1, so the rows are there)
    the stacks of a stage                  D_j = sum (p1 + p2) differ; stack j's FIRST convolution (and that pair's residual)
                                           reads its input with the extra lag e_j = max D - D_j, so the mean adds aligned rows
    upsampling stage of stride s           d_out = d_in * s + E, E = max(P, (k7 - 1) / 2), P = (K_T - s) / 2: with that both
                                           paths read tokens already seen, and the stage is one polyphase contraction
                                           (``fused_stage_weight``)

Every layer's output is stored as 0.0 outside the utterance (the reference zero-pads every layer at the utterance's edges;
zeros pass through LeakyReLU and sin(h) + h), input rows at or beyond the end are flush rows that are never loaded, and a
slot is done ``flush_frames = ceil(delay_samples / hop)`` frames after its last one.  csrc/sconv_sym.hip is the kernel,
kantts._hip.nc_emit the emission rule; ``synthesize`` and ``play_many`` are the base class's, fed ``flush_frames``, ``end``
and that rule.

    v = ChunkedNCVocoder(generator, slots=S, graph=True)      # generator: causal=False, eval, on the device
    v.delay_samples, v.flush_frames                           # ChunkedNCVocoder.delay_of(generator) needs no device
    wav = v.step(mel, rows=[8, 3, 0, 8], end=[-1, 40, -1, 17])  # end: frames of the slot's utterance, -1 while open
    for wav in v.synthesize(mel_full, chunk_frames=8): ...    # chunks add up to T * hop samples
    for index, wav in v.play_many(mels, chunk_frames=8): ...
"""
import torch

import kantts._hip as hip
from kantts._hip import ops
from kantts.models.hifigan.chunked import ChunkedVocoder, slot_ints
from kantts.models.hifigan.layers import Conv1d, ConvTranspose1d, effective_weight


def stage_geometry(K_T, s, k7):
    """(P, E, J) of an upsampling stage: transposed kernel ``K_T`` at stride ``s`` with padding P = (K_T - s) // 2 and
    (``k7`` not None) the symmetric k7 convolution over the nearest-repeated signal.  E: delay the stage adds, in output
    samples; J: input tokens per output row."""
    P = (K_T - s) // 2
    p7 = 0 if k7 is None else (k7 - 1) // 2
    E = max(P, p7)
    J = 1 + (K_T - 1 + E - P) // s
    if k7 is not None:
        J = max(J, 1 + -(-(E + p7) // s))
    return P, E, J


def fused_stage_weight(w_t, w7, s):
    """Both paths of a symmetric upsampling stage as ONE polyphase contraction: w_t (Cin, Cout, K_T) of the transposed
    convolution, w7 (Cout, Cin, k7) of the convolution over the repeated signal (or None) -> w (Cin, Cout, J * s) with
    w[ci, co, r + j * s] the coefficient of stream token q - j in stream sample q * s + r, the output stream being
    d_in * s + E samples late.  True sample m = q' s + r - E (q' = q - d_in) and true token q' - j meet at tap
    r - (E - P) + j s of the transposed kernel; tap k of the k7 convolution reads token q' + floor((r - E + k - p7) / s)."""
    Cin, Cout, K_T = w_t.shape
    k7 = None if w7 is None else int(w7.shape[2])
    P, E, J = stage_geometry(K_T, s, k7)
    w = w_t.new_zeros(Cin, Cout, J * s)
    for j in range(J):
        for r in range(s):
            tap = r - (E - P) + j * s
            if 0 <= tap < K_T:
                w[:, :, r + j * s] += w_t[:, :, tap]
    if w7 is not None:
        p7 = (k7 - 1) // 2
        for k in range(k7):
            for r in range(s):
                j = -((r - E + k - p7) // s)
                w[:, :, r + j * s] += w7[:, :, k].t()
    return w


def plan_delays(g):
    """The delay table of a non-causal generator, from shapes alone: a list of (name, rows per frame, delay) for the output
    of conv_pre, of every stage's upsampling and residual stacks, and of conv_post."""
    table = []
    k = g.conv_pre.conv1d
    d = (k.kernel_size[0] - 1) * k.dilation[0] // 2
    mul = 1
    table.append(("conv_pre", mul, d))
    for i, s in enumerate(int(x) for x in g.upsample_scales):
        K_T = g.transpose_upsamples[i][1].deconv.kernel_size[0]
        k7 = g.repeat_upsamples[i][2].conv1d.kernel_size[0] if g.repeat_upsample else None
        d = d * s + stage_geometry(K_T, s, k7)[1]
        mul *= s
        table.append(("stage%d.up" % i, mul, d))
        d += max(_stack_delay(blk) for blk in g.conv_blocks[i * g.num_kernels:(i + 1) * g.num_kernels])
        table.append(("stage%d.stacks" % i, mul, d))
    k = g.conv_post.conv1d
    d += (k.kernel_size[0] - 1) * k.dilation[0] // 2
    table.append(("conv_post", mul, d))
    return table


def _pad_of(m):
    c = m.conv1d
    return (c.kernel_size[0] - 1) * c.dilation[0] // 2


def _stack_delay(blk):
    return sum(_pad_of(c1) + _pad_of(c2) for c1, c2 in zip(blk.convs1, blk.convs2))


class ChunkedNCVocoder(ChunkedVocoder):
    """Chunk-by-chunk inference of a non-causal single-band ``Generator`` on ``slots`` independent utterances: the
    launches of ``ChunkedVocoder`` (one per layer, the state carried inside them) on kantts_sconv_sym_rows_launch.

    The waveform comes ``delay_samples`` late: a step that advances a slot from ``pos`` by ``n`` frames holds the true
    samples [max(0, pos * hop - delay), min((pos + n) * hop - delay, end * hop)) (``kantts._hip.nc_emit``) and 0.0
    elsewhere; a slot is done after ``end + flush_frames`` frames and an utterance's chunks add up to ``end * hop`` samples.

    State: the arena of the base class, a layer keeping ``(k - 1) * dilation + lag`` rows, and behind the layers one int32
    word per slot, the frames consumed so far -- ping-pong with the rest (written by the state workgroups of conv_pre's
    launch, read by every launch of the step), so a zeroed state is a fresh slot and captured steps stay valid across
    resets.  ``rows`` and ``end`` live in persistent device buffers the captured launches read.

    Refused at construction: causal generators (``ChunkedVocoder`` plays them), NSF generators
    (kantts.models.hifigan.chunked_nc_nsf.ChunkedNCNSFVocoder plays them), ``out_channels > 1``,
    ``training``, upsampling kernels with (kernel - stride) odd or below 0, even convolution kernels, and whatever the
    layer contract declines."""

    _plays_noncausal = True
    _end_kw, _solo = "end", True
    _conv_cls, _up_cls = Conv1d, ConvTranspose1d

    def __init__(self, generator, slots=1, graph=True, max_graphs=8):
        if getattr(generator, "causal", False):
            raise ValueError("ChunkedNCVocoder plays non-causal generators (causal=False); a causal one needs no delay: "
                             "use ChunkedVocoder")
        if generator.nsf_enable and not self._plays_nsf:  # chunked_nc_nsf.ChunkedNCNSFVocoder plays them
            raise NotImplementedError("ChunkedNCVocoder: non-causal NSF generators are not supported (the symmetric "
                                      "source_downs and the excitation's delay are not built)")
        if generator.out_channels != 1:
            raise NotImplementedError("ChunkedNCVocoder: out_channels > 1 (non-causal multi-band) is not supported")
        super().__init__(generator, slots=slots, graph=graph, max_graphs=max_graphs)
        self._end = torch.full((self.slots,), -1, device=self.device, dtype=torch.int32)
        self._arena_i32 = self.arena.view(torch.int32)

    @staticmethod
    def delay_of(generator):
        """Delay of the waveform in samples, from the generator's shapes alone (no device)."""
        return plan_delays(generator)[-1][2]

    # ---- geometry
    def _stage_taps(self, g, i, s):
        d = g.transpose_upsamples[i][1].deconv
        K_T = d.kernel_size[0]
        if K_T < s or (K_T - s) % 2 or g.transpose_upsamples[i][1].padding != (K_T - s) // 2:
            raise NotImplementedError("ChunkedNCVocoder: upsampling kernel %d at stride %d needs kernel >= stride, "
                                      "(kernel - stride) even and padding (kernel - stride) / 2" % (K_T, s))
        k7 = g.repeat_upsamples[i][2].conv1d.kernel_size[0] if g.repeat_upsample else None
        return stage_geometry(K_T, s, k7)[2]

    def _stage_weight(self, g, i, s):
        up = g.transpose_upsamples[i][1].deconv
        w7 = b = None
        if g.repeat_upsample:
            c = g.repeat_upsamples[i][2].conv1d
            w7, b = effective_weight(c), c.bias
        w = fused_stage_weight(effective_weight(up), w7, s)
        if up.bias is not None:
            b = up.bias if b is None else b + up.bias
        return w, b

    def _plan_extra(self, g):
        """Delay, lag and residual lag of every layer, and the state layout that follows from them."""
        ups = [upl for _, _, upl, _ in self.stages]
        for L in self.layers:
            if not any(L is u for u in ups) and (L.K - 1) * L.step % 2:
                raise NotImplementedError("ChunkedNCVocoder: layer %s has an even kernel (no symmetric padding)" % L.name)
            L.lag, L.res_lag, L.res_from, L.sub = 0, 0, None, 1
        pad = lambda L: L.H // 2
        d = pad(self.pre)
        self.pre.delay = d
        for i, (s, Cout, upl, stacks) in enumerate(self.stages):
            K_T = g.transpose_upsamples[i][1].deconv.kernel_size[0]
            k7 = g.repeat_upsamples[i][2].conv1d.kernel_size[0] if g.repeat_upsample else None
            d = d * s + stage_geometry(K_T, s, k7)[1]
            upl.delay, upl.sub = d, s
            Dj = [sum(pad(c1) + pad(c2) for c1, c2 in pairs) for pairs in stacks]
            for pairs, D in zip(stacks, Dj):
                dd = d
                for n, (c1, c2) in enumerate(pairs):
                    if pad(c2) > pad(c1):
                        raise NotImplementedError("ChunkedNCVocoder: %s is wider than %s: the residual would lie beyond the "
                                                  "state %s keeps" % (c2.name, c1.name, c1.name))
                    c1.lag = max(Dj) - D if n == 0 else 0  # the alignment of the stacks, at the first convolution
                    c1.delay = dd + c1.lag + pad(c1)
                    c2.delay = dd = c1.delay + pad(c2)
                    c2.res_from, c2.res_lag = c1, c1.lag + pad(c1) + pad(c2)
                assert dd == d + max(Dj)
            d += max(Dj)
        self.post.delay = d + pad(self.post)
        self.delay_samples = self.post.delay
        assert self.delay_samples == plan_delays(g)[-1][2]
        self.flush_frames = -(-self.delay_samples // self.hop)
        off = 0
        for L in self.layers:
            L.Hs = L.H + L.lag
            L.off = off
            off += L.Hs * L.Cin
        self._pos_off = off  # one int32 word per slot; the arena's slot stride stays a multiple of 4 floats
        self.state_floats = off + 4
        if not hip.sconv_sym_entry_points():  # the first look at the library: behind every refusal, before anything is packed
            raise RuntimeError("ChunkedNCVocoder: the loaded library has no kantts_sconv_sym_rows_launch")

    # ---- launches
    def _conv(self, L, x, parity, res=None, rows=None, row_mul=1, zero_tail=False):
        S, T, _ = x.shape
        out = torch.empty((S, T, L.N), device=x.device, dtype=torch.float32)
        ss = self.arena.shape[2]
        hin = hout = None
        if L.Hs:
            hin = self.arena[parity, 0, L.off:L.off + L.Hs * L.Cin]
            hout = self.arena[1 - parity, 0, L.off:L.off + L.Hs * L.Cin]
        kw = {}
        if res is not None:
            R = L.res_from
            if R is None:  # an up-layer's excitation: produced as late as the layer's output, read at res_lag = 0
                kw = dict(res=res)
            else:
                kw = dict(res=res, res_hist=self.arena[parity, 0, R.off:R.off + R.Hs * R.Cin], res_hist_ss=ss,
                          res_hist_rows=R.Hs, res_lag=L.res_lag)
        first = L is self.pre
        ok = hip.sconv_sym(x, hin, hout, L.w, out, S=S, Tc=T, Cin=L.Cin, N=L.N, K=L.K, step=L.step, hist_ss=ss,
                           precision=self.precision, rows=rows, end=self._end, row_mul=row_mul,
                           pos_in=self._arena_i32[parity, 0, self._pos_off:], pos_ss=ss,
                           pos_out=self._arena_i32[1 - parity, 0, self._pos_off:] if first else None,
                           delay=L.delay, sub=L.sub, lag=L.lag, in_end=first, bias=L.bias, in_leaky=L.in_leaky,
                           zero_tail=zero_tail, **kw)
        if not ok:
            raise RuntimeError("kantts_sconv_sym_rows_launch declined layer %s it was planned for" % L.name)
        return out

    def reset(self, slot=None):
        """Zero state for one slot (others untouched) or for all, and its end open again."""
        super().reset(slot)
        if slot is None:
            self._end.fill_(-1)
        else:
            self._end[int(slot)] = -1

    def _set_end(self, end):
        vals = slot_ints(end, "end", self.slots)
        self._end.copy_(end if torch.is_tensor(end) else torch.tensor([max(e, -1) for e in vals], dtype=torch.int32))

    def step(self, mel, rows=None, end=None):
        """mel (slots, C_mel, Tc) -> wav (slots, 1, Tc * hop), ``delay_samples`` late (see the class).  ``rows`` as in
        ``ChunkedVocoder.step`` (None: every slot takes Tc frames).  ``end``: ``slots`` ints or an integer tensor, the frame
        count of each slot's utterance, -1 while it is open; None keeps what was given before (``reset`` opens it).  It must
        be given no later than the first step that feeds a frame at or beyond it; frames of ``mel`` at or beyond it are
        flush frames and are not read."""
        if mel.dim() != 3 or mel.shape[0] != self.slots or mel.shape[1] != self._step_channels or mel.shape[2] < 1:
            raise ValueError("mel must be (slots=%d, %d, Tc >= 1), got %s" % (self.slots, self._step_channels, tuple(mel.shape)))
        if end is not None:
            self._set_end(end)
        return super().step(mel, rows=[int(mel.shape[2])] * self.slots if rows is None else rows)

    def _end_of(self, pos, n, T):
        return T

    def _emitted(self, pos, n, T):
        return hip.nc_emit(pos, n, T, self.delay_samples, self.hop)

    def _solo_end(self, slot, pos, n, T):
        """The end is kept between steps: written once, for ``slot`` alone, so the other slots' ends stay what was given."""
        if pos == 0:
            self._end[slot] = T
        return {}
