"""Chunked inference of NON-CAUSAL NSF HiFi-GAN generators: the delay / flush machinery of ``ChunkedNCVocoder`` plus the
excitation state of ``ChunkedNSFVocoder``, joined by two launches per step (csrc/nsf_source_sym.hip).

The excitation itself is not delayed: it is made from f0 and voicing, sample for sample, and the source module looks neither
back nor ahead.  What the symmetric network needs of it is

* kantts_nsf_source_end_rows: the sine source stopped at the utterance's end -- flush frames draw no noise and move neither
  the phase nor the cursor, so the excitation of an utterance is the same bits however its end falls into the chunks;
* kantts_nsf_downs_sym_rows: every ``source_downs`` convolution (kernel 2 u, stride u, padding u // 2) read with the lag

      lag_i = D_i * u_i + p_i          D_i: delay of stage i's up-layer output (rows at its rate), p_i = u_i // 2

  which puts the convolution's true row m = q - D_i into row q of the stream, where the up-layer's launch adds it as its
  ``res`` (at res_lag 0).  The zeros before the utterance are the zeroed history, the zeros behind it are not loaded, and
  rows outside the utterance are stored as 0.0 by the up-layer's own window.  The history is the last
  ``excitation_history = max_i lag_i`` samples of the excitation per slot (the deepest stage's delay: 3321 samples of the
  shipped geometry).

    v = ChunkedNCNSFVocoder(generator, slots=S, graph=True, seed=0)   # generator: causal=False with nsf_params, eval
    v.delay_samples, v.flush_frames, v.excitation_history             # ChunkedNCNSFVocoder.delay_of / plan_lags: no device
    wav = v.step(feats, rows=[8, 3, 0, 8], end=[-1, 40, -1, 17])      # feats (S, C_mel + 2, Tc): f0 (Hz) and voicing last
    for wav in v.synthesize(feats_full, chunk_frames=8, slot=0, key=0): ...   # chunks add up to T * hop samples
    for index, wav in v.play_many(feats_list, chunk_frames=8): ...            # utterance i plays as key=i

The source module adds no delay: ``delay_samples`` is ``ChunkedNCVocoder``'s for the same network (3424 samples = 18 frames
shipped), and emission is ``kantts._hip.nc_emit``.
"""
import torch

import kantts._hip as hip
from kantts.models.hifigan.chunked import ChunkedVocoder
from kantts.models.hifigan.chunked_nc import ChunkedNCVocoder, plan_delays
from kantts.models.hifigan.chunked_nsf import _Excitation
from kantts.models.hifigan.layers import Conv1d


def down_geometry(hop, scales):
    """[(u, k, p)] of the symmetric ``source_downs`` of a generator: stride, kernel and padding of every stage's."""
    out, u = [], int(hop)
    for s in scales:
        u //= int(s)
        out.append((u, 2 * u, u // 2) if u > 1 else (1, 1, 0))
    return out


def plan_lags(g):
    """The lag of every ``source_downs`` convolution of a non-causal NSF generator, from shapes alone:
    lag_i = D_i * u_i + p_i with D_i the delay of stage i's up-layer output (``plan_delays``)."""
    scales = [int(s) for s in g.upsample_scales]
    hop = 1
    for s in scales:
        hop *= s
    delays = {name: d for name, _, d in plan_delays(g)}
    return [delays["stage%d.up" % i] * u + p for i, (u, _, p) in enumerate(down_geometry(hop, scales))]


class ChunkedNCNSFVocoder(_Excitation, ChunkedNCVocoder):
    """``ChunkedNCVocoder`` for non-causal single-band generators WITH a source module (``nsf_params``).

    ``step`` takes (slots, C_mel + 2, Tc) features, f0 in Hz and voicing last, with ``rows`` and ``end`` as in
    ``ChunkedNCVocoder.step``; frames at or beyond a slot's end are flush frames and are read by no launch.  Per slot it
    carries, beside the arena, the source words of ``ChunkedNSFVocoder`` (2, slots, 36) and the last
    ``excitation_history`` samples of the excitation (2, slots, excitation_history), both ping-pong with the arena's parity.

    Refused at construction, before anything is packed or launched: what ``ChunkedNCVocoder`` refuses apart from NSF (causal
    generators among it), generators without a source module, what ``ChunkedNSFVocoder`` refuses about the source module
    (``nb_harmonics + 1 > 16``, ``upsample_ratio != hop``, a projection that is not 1x1, the stage count), ``source_downs[i]``
    that is not ``Conv1d(1, C_i, 2 u, u, padding=u // 2)`` (the 1x1 convolution for ``u == 1``), and odd ``u > 1``, whose
    lengths the reference's own forward cannot add."""

    _plays_nsf = True

    def __init__(self, generator, slots=1, graph=True, seed=0, given_noise=False, max_graphs=8):
        self.seed = int(seed)
        self.given_noise = bool(given_noise)
        super().__init__(generator, slots=slots, graph=graph, max_graphs=max_graphs)
        self._pack_source(generator, self.excitation_history)
        self.reset()

    delay_of = staticmethod(ChunkedNCVocoder.delay_of)

    def _plan_extra(self, g):
        if not g.nsf_enable:
            raise ValueError("ChunkedNCNSFVocoder needs a generator with a source module (nsf_params); "
                             "ChunkedNCVocoder plays the others")
        self._plan_source(g, "ChunkedNCNSFVocoder", "kantts_nsf_downs_sym_rows")
        self._down_geom = []
        geom = down_geometry(self.hop, self.scales)
        for i, ((s, Cout, _, _), m, (u, k, p)) in enumerate(zip(self.stages, g.source_downs, geom)):
            if u > 1 and u % 2:
                raise NotImplementedError("ChunkedNCNSFVocoder: source_downs[%d] has the odd stride %d: kernel %d with padding "
                                          "%d gives one row fewer than the stage it is added to" % (i, u, k, p))
            if not isinstance(m, Conv1d) or getattr(m, "causal", False):
                raise ValueError("ChunkedNCNSFVocoder: source_downs[%d] is not a symmetric Conv1d" % i)
            c = m.conv1d
            if (c.in_channels != 1 or c.out_channels != Cout or c.kernel_size[0] != k or c.stride[0] != u or c.padding[0] != p
                    or c.dilation[0] != 1 or c.groups != 1 or k > hip.NSF_MAX_K):
                raise NotImplementedError(
                    "ChunkedNCNSFVocoder: source_downs[%d] (Cin %d, Cout %d, k %d, stride %d, padding %d) is not the 1 -> %d "
                    "convolution with kernel %d, stride %d and padding %d kantts_nsf_downs_sym_rows runs"
                    % (i, c.in_channels, c.out_channels, c.kernel_size[0], c.stride[0], c.padding[0], Cout, k, u, p))
            self._down_geom.append((u, k, Cout))
        super()._plan_extra(g)  # the delays of the network (and its own refusals): the lags follow from the up-layers'
        self.lags = [upl.delay * u + p for (_, _, upl, _), (u, _, p) in zip(self.stages, geom)]
        assert self.lags == plan_lags(g)
        if not hip.nsf_sym_entry_points():
            raise RuntimeError("ChunkedNCNSFVocoder: the loaded library has no kantts_nsf_source_end_rows / "
                               "kantts_nsf_downs_sym_rows")
        self.excitation_history = max(self.lags)

    # ------------------------------------------------------------------------------------------------------------
    def reset(self, slot=None, key=0, phase0=None):
        """``ChunkedNCVocoder.reset`` and ``ChunkedNSFVocoder.reset`` in one: zero state (arena, position, excitation
        history) and an open end for one slot or for all, and the identity of the utterance that starts there -- the noise
        key from ``(seed, key)``, the initial phases from the same hash or ``phase0``."""
        super().reset(slot)
        self._reset_excitation(slot, key, phase0)

    def _run(self, feats, parity, rows=None):
        """The launches of one step: the source, its down-convolutions, then ``ChunkedVocoder._run`` on the symmetric
        layers with every stage's excitation as the ``res`` of its up-layer.  Reads half ``parity`` of the arena, of the
        source words and of the excitation history, writes the other."""
        S, _, Tc = feats.shape
        hop = self.hop
        pos = dict(end=self._end, pos_in=self._arena_i32[parity, 0, self._pos_off:], pos_ss=self.arena.shape[2])
        with torch.no_grad():
            f0, uv = feats[:, -2, :].contiguous(), feats[:, -1, :].contiguous()
            e = torch.empty((S, Tc * hop, 1), device=feats.device, dtype=torch.float32)
            ok = hip.nsf_source_end(f0, uv, self._nsf_state[parity], self._nsf_state[1 - parity], self._src_w, e, S=S, Tc=Tc,
                                    hop=hop, H1=self.H1, sr=self.sr, alpha=self.alpha, sigma=self.sigma, bias=self._src_b,
                                    noise=self._step_noise(Tc), rows=rows, **pos)
            outs = [torch.empty((S, Tc * hop // u, C), device=feats.device, dtype=torch.float32) for u, _, C, _, _ in self._downs]
            ok = ok and hip.nsf_downs_sym(e, self._nsf_hist[parity], self._nsf_hist[1 - parity], self._downs, self.lags, outs,
                                          S=S, Tc=Tc, hop=hop, hist_rows=self._hh, hist_ss=self._hist_ss, rows=rows, **pos)
            if not ok:
                raise RuntimeError("the NSF source kernels declined a generator they were planned for")
        return ChunkedVocoder._run(self, feats[:, :-2, :], parity, rows, stage_res=outs)

    def step(self, feats, rows=None, end=None, noise=None):
        """feats (slots, C_mel + 2, Tc) -> wav (slots, 1, Tc * hop), ``delay_samples`` late; ``rows`` and ``end`` as in
        ``ChunkedNCVocoder.step``.  ``noise`` (slots, Tc * hop, H + 1) fp32: required with ``given_noise=True`` (frames at or
        beyond a slot's count, and flush frames, are not read), a ValueError without it."""
        self._take_noise(feats, noise)
        try:
            return super().step(feats, rows=rows, end=end)
        finally:
            self._noise = None
