"""Chunked inference of causal NSF HiFi-GAN generators: ``ChunkedVocoder`` plus a streamed sine excitation.

``SourceModule.excitation`` works on a whole utterance (an fp32 running sum for the phase, one draw of initial phases and
one draw of noise per utterance), so it cannot resume across chunks.  ``ChunkedNSFVocoder`` replaces it, for inference, by
two launches per step (csrc/nsf_source.hip) that carry their own state per slot:

* kantts_nsf_source_rows: f0 and voicing of the chunk's frames -> the projected excitation.  The phase of every harmonic
  is a 32-bit fixed-point accumulator (exact, so independent of where the chunks are cut), the noise is a counter-based
  Gaussian keyed by (key of the utterance, harmonic, absolute sample index);
* kantts_nsf_downs_rows: every ``source_downs`` convolution, with the last ``2 * u_0 - 1`` excitation samples carried.

Each stage's down-sampled excitation goes into the ``res`` argument of that stage's polyphase up-layer launch, where
``Generator.forward`` adds it.  Everything else is the base class.

    v = ChunkedNSFVocoder(generator, slots=S, graph=True, seed=0)
    wav = v.step(feats, rows=None)          # feats (S, C_mel + 2, Tc): the last two channels are f0 (Hz) and voicing
    v.reset(slot=None, key=0, phase0=None)  # also names the utterance: (seed, key) fixes its noise and initial phases
    for wav in v.synthesize(feats_full, chunk_frames=8, slot=0, key=0): ...
    for index, wav in v.play_many(feats_list, chunk_frames=8): ...   # utterance i plays with key=i

The excitation is not the reference's sample for sample: frames are indexed exactly (sample n belongs to frame n // hop,
where ``interpolate``'s float scale can pick the neighbouring frame for hops that are no power of two), and phases and
noise come from the hash of csrc/common.h instead of torch's generator.  ``given_noise=True`` takes the noise from the
caller (``step(feats, noise=...)``, (S, Tc * hop, H + 1)) -- the hook that lets tests compare with the module's arithmetic.
"""
import math

import torch

import kantts._hip as hip
from kantts.models.hifigan.chunked import ChunkedVocoder
from kantts.models.hifigan.layers import CausalConv1d, Conv1d, effective_weight

_M64 = (1 << 64) - 1


def rng_mix(seed, blk):
    """kantts_rng_mix of csrc/common.h on Python ints."""
    z = (seed + blk * 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def slot_key(seed, key):
    """The 64-bit noise key of utterance ``key`` under ``seed``."""
    return rng_mix(rng_mix(int(seed) & _M64, 0x4E5346), int(key) & _M64)


def initial_phases(key64, H1):
    """phase0 (H1) fp32, uniform in [-pi, pi) from the same hash (blocks >= 2^63: the noise uses blocks 8 * n + i below
    that), harmonic 0 at 0 as in the reference."""
    vals = [0.0] + [((rng_mix(key64, (1 << 63) + h) >> 40) / 16777216.0 * 2.0 - 1.0) * math.pi for h in range(1, H1)]
    return torch.tensor(vals, dtype=torch.float32)


def initial_state(seed, key, H1, phase0=None):
    """The KANTTS_NSF_STATE_WORDS int32 words (include/kantts_hip.h) of a slot at the start of utterance ``key``: zero
    phase and cursor, the initial phases (``phase0``, or from the hash) and the noise key."""
    k64 = slot_key(seed, key)
    if phase0 is None:
        p0 = initial_phases(k64, H1)
    else:
        p0 = torch.as_tensor(phase0, dtype=torch.float32).reshape(-1).cpu().contiguous()
        if p0.numel() != H1:
            raise ValueError("phase0 must hold %d values, got %d" % (H1, p0.numel()))
    words = torch.zeros(hip.NSF_STATE_WORDS, dtype=torch.int32)
    words[16:16 + H1] = p0.view(torch.int32)
    lo, hi = k64 & 0xFFFFFFFF, k64 >> 32
    words[34] = lo - (1 << 32) if lo >= (1 << 31) else lo
    words[35] = hi - (1 << 32) if hi >= (1 << 31) else hi
    return words


class _Excitation:
    """What a chunked vocoder carries for the source module, whichever network it feeds (``ChunkedNSFVocoder`` here,
    kantts.models.hifigan.chunked_nc_nsf.ChunkedNCNSFVocoder): the plan and the snapshot of the source module, the per-slot
    source words and excitation history (ping-pong with the arena), the identity of an utterance and the noise argument.
    The class that mixes it in sets ``seed`` and ``given_noise`` before the base constructor runs, ``_down_geom`` in its
    ``_plan_extra``, and calls ``_pack_source`` after it."""

    def _plan_source(self, g, who, launch):
        """The refusals about the source module, from shapes alone; sets H1, sr, alpha, sigma and the step's channels."""
        sm = g.source_module
        self.H1 = int(sm.nb_harmonics) + 1
        self.sr, self.alpha, self.sigma = float(sm.sampling_rate), float(sm.alpha), float(sm.sigma)
        if self.H1 > hip.NSF_MAX_H1:
            raise NotImplementedError("%s: nb_harmonics + 1 = %d harmonics, kantts_nsf_source_rows takes %d"
                                      % (who, self.H1, hip.NSF_MAX_H1))
        if int(sm.upsample_ratio) != self.hop:
            raise NotImplementedError("%s: the source module's upsample_ratio %d is not the hop %d"
                                      % (who, int(sm.upsample_ratio), self.hop))
        c = sm.ffn[0]
        if c.in_channels != self.H1 or c.out_channels != 1 or c.kernel_size[0] != 1:
            raise NotImplementedError("%s: the source projection is not a 1x1 convolution H + 1 -> 1" % who)
        if len(self.stages) > hip.NSF_MAX_STAGES or len(g.source_downs) != len(self.stages):
            raise NotImplementedError("%s: %d stages / %d source_downs, %s takes one per stage and at most %d"
                                      % (who, len(self.stages), len(g.source_downs), launch, hip.NSF_MAX_STAGES))
        self._step_channels = self.in_channels + 2

    def _pack_source(self, g, hist_rows):
        """Snapshot of the source projection and of every ``source_downs`` (tap-major), and the state buffers: the source
        words (2, slots, 36) and ``hist_rows`` excitation samples per slot (2, slots, hist_rows)."""
        dev = self.device
        with torch.no_grad():
            c = g.source_module.ffn[0]
            self._src_w = effective_weight(c).detach().float().reshape(-1).contiguous().clone()
            self._src_b = None if c.bias is None else c.bias.detach().float().contiguous().clone()
            self._downs = []
            for (u, k, C), m in zip(self._down_geom, g.source_downs):
                w = effective_weight(m.conv1d).detach().float()  # (C, 1, k)
                b = m.conv1d.bias
                self._downs.append((u, k, C, w[:, 0, :].t().contiguous().clone(),
                                    None if b is None else b.detach().float().contiguous().clone()))
        self._hh = int(hist_rows)
        self._hist_ss = max(self._hh, 1)
        self._nsf_state = torch.zeros(2, self.slots, hip.NSF_STATE_WORDS, device=dev, dtype=torch.int32)
        self._nsf_hist = torch.zeros(2, self.slots, self._hist_ss, device=dev, dtype=torch.float32)
        self._noise = None      # the noise of the step being issued (given_noise, eager)
        self._noise_bufs = {}   # Tc -> static noise buffer of the captured steps

    def _reset_excitation(self, slot, key, phase0):
        words = initial_state(self.seed, key, self.H1, phase0)
        words = words.to(self.device)
        if slot is None:
            self._nsf_state.copy_(words.expand_as(self._nsf_state))
            self._nsf_hist.zero_()
        else:
            self._nsf_state[:, int(slot)] = words
            self._nsf_hist[:, int(slot)].zero_()

    def _assign(self, slot, index):
        self.reset(slot, key=index)

    def _save_state(self):
        return (self.arena.clone(), self._nsf_state.clone(), self._nsf_hist.clone())

    def _restore_state(self, saved):
        self.arena.copy_(saved[0])
        self._nsf_state.copy_(saved[1])
        self._nsf_hist.copy_(saved[2])

    def _noise_buf(self, Tc):
        buf = self._noise_bufs.get(Tc)
        if buf is None:
            buf = self._noise_bufs[Tc] = torch.zeros(self.slots, Tc * self.hop, self.H1, device=self.device)
        return buf

    def _step_noise(self, Tc):
        """The noise operand of the source launch being issued: None unless the vocoder was built with ``given_noise``."""
        if not self.given_noise:
            return None
        return self._noise_buf(Tc) if self.graph else self._noise

    def _take_noise(self, feats, noise):
        """Validate the ``noise`` argument of a step and put it where the step's source launch reads it."""
        if self.given_noise != (noise is not None):
            raise ValueError("noise must be given when, and only when, the vocoder was built with given_noise=True")
        if noise is not None:
            want = (self.slots, (feats.shape[2] if feats.dim() == 3 else 0) * self.hop, self.H1)
            if tuple(noise.shape) != want:
                raise ValueError("noise must be %s, got %s" % (want, tuple(noise.shape)))
            noise = noise.to(device=self.device, dtype=torch.float32).contiguous()
            if self.graph:
                self._noise_buf(int(feats.shape[2])).copy_(noise)
            else:
                self._noise = noise


class ChunkedNSFVocoder(_Excitation, ChunkedVocoder):
    """``ChunkedVocoder`` for causal single-band generators WITH a source module (``nsf_params``).

    ``step`` takes the features ``Generator.forward`` takes: (slots, C_mel + 2, Tc), f0 in Hz and voicing last.  Per slot
    it carries, beside the convolution state, the running phase, the sample cursor, the initial phases and the noise key
    (one int32 buffer (2, slots, 36), ping-pong with the arena) and the excitation history (2, slots, 2 * u_0 - 1).

    Refused at construction, before anything is packed: what the base refuses, generators without a source module,
    ``nb_harmonics + 1 > 16``, more than 8 stages, and ``source_downs`` that are not the reference's (one input channel,
    kernel ``2 * u`` and stride ``u = hop / prod(scales[:i+1])``, the 1x1 convolution for ``u == 1``, ``channels`` of the
    stage)."""

    _plays_nsf = True

    def __init__(self, generator, slots=1, graph=True, seed=0, given_noise=False, max_graphs=8):
        self.seed = int(seed)
        self.given_noise = bool(given_noise)
        super().__init__(generator, slots=slots, graph=graph, max_graphs=max_graphs)
        self._pack_source(generator, max(k for _, k, _ in self._down_geom) - 1)
        self.reset()

    def _plan_extra(self, g):
        if not g.nsf_enable:
            raise ValueError("ChunkedNSFVocoder needs a generator with a source module (nsf_params); "
                             "ChunkedVocoder plays the others")
        self._plan_source(g, "ChunkedNSFVocoder", "kantts_nsf_downs_rows")
        self._down_geom = []
        u = self.hop
        for i, ((s, Cout, _, _), m) in enumerate(zip(self.stages, g.source_downs)):
            u //= s
            k = 2 * u if u > 1 else 1
            if not isinstance(m, CausalConv1d if u > 1 else Conv1d):
                raise ValueError("ChunkedNSFVocoder: source_downs[%d] is not causal" % i)
            c = m.conv1d
            if (c.in_channels != 1 or c.out_channels != Cout or c.kernel_size[0] != k or c.stride[0] != u
                    or c.dilation[0] != 1 or c.groups != 1 or (u == 1 and c.padding[0] != 0) or k > hip.NSF_MAX_K):
                raise NotImplementedError(
                    "ChunkedNSFVocoder: source_downs[%d] (Cin %d, Cout %d, k %d, stride %d) is not the 1 -> %d convolution "
                    "with kernel %d and stride %d kantts_nsf_downs_rows runs"
                    % (i, c.in_channels, c.out_channels, c.kernel_size[0], c.stride[0], Cout, k, u))
            self._down_geom.append((u, k, Cout))

    # ------------------------------------------------------------------------------------------------------------
    def reset(self, slot=None, key=0, phase0=None):
        """Zero state for one slot (others untouched) or for all -- convolution state, running phase, sample cursor and
        excitation history -- and the identity of the utterance that starts there: the noise key from ``(seed, key)``,
        the initial phases from the same hash (uniform in [-pi, pi), harmonic 0 at 0) or ``phase0`` ((H + 1) floats)."""
        super().reset(slot)
        self._reset_excitation(slot, key, phase0)

    def _run(self, feats, parity, rows=None):
        """The launches of one step: the source, its down-convolutions, then the base class's with every stage's
        excitation as the ``res`` of its up-layer.  Reads half ``parity`` of every state buffer, writes the other."""
        S, _, Tc = feats.shape
        hop = self.hop
        with torch.no_grad():
            f0, uv = feats[:, -2, :].contiguous(), feats[:, -1, :].contiguous()
            noise = self._step_noise(Tc)
            e = torch.empty((S, Tc * hop, 1), device=feats.device, dtype=torch.float32)
            ok = hip.nsf_source(f0, uv, self._nsf_state[parity], self._nsf_state[1 - parity], self._src_w, e, S=S, Tc=Tc,
                                hop=hop, H1=self.H1, sr=self.sr, alpha=self.alpha, sigma=self.sigma, bias=self._src_b,
                                noise=noise, rows=rows)
            outs = [torch.empty((S, Tc * hop // u, C), device=feats.device, dtype=torch.float32) for u, _, C, _, _ in self._downs]
            ok = ok and hip.nsf_downs(e, self._nsf_hist[parity], self._nsf_hist[1 - parity], self._downs, outs, S=S, Tc=Tc,
                                      hop=hop, hist_ss=self._hist_ss, rows=rows)
            if not ok:
                raise RuntimeError("the NSF source kernels declined a generator they were planned for")
        return super()._run(feats[:, :-2, :], parity, rows, stage_res=outs)

    def step(self, feats, rows=None, noise=None):
        """feats (slots, C_mel + 2, Tc) -> wav (slots, 1, Tc * hop); ``rows`` as in ``ChunkedVocoder.step``.  ``noise``
        (slots, Tc * hop, H + 1) fp32: required with ``given_noise=True`` (frames at and after a slot's count are not
        read), a ValueError without it."""
        self._take_noise(feats, noise)
        try:
            return super().step(feats, rows=rows)
        finally:
            self._noise = None
