"""Chunked inference of causal MULTI-BAND HiFi-GAN generators: ``ChunkedVocoder`` plus a PQMF synthesis that can be cut at
a chunk boundary.

A multi-band generator (``out_channels = B > 1``, then ``PQMF.synthesis``) runs its convolution stack at 1 / B of the sample
rate.  Two things keep ``ChunkedVocoder`` from playing it: a ``conv_post`` with B outputs, and the synthesis bank, which is
symmetric -- low-rate output row ``q`` needs the sub-band rows ``q - D .. q + D``, ``D = ceil((taps / 2) / B)`` (8 for the
default 62 taps and 4 bands), so it looks AHEAD and nothing causal can carry that as history.  ``ChunkedMBVocoder`` replaces
the last launches of a step by ONE (csrc/mb_tail.hip, kantts_mb_tail_rows: conv_post, tanh and the streamed synthesis) that
holds back the rows whose future it has not seen: per slot it carries the last ``2 D`` sub-band rows and a count of pending
rows, emits late, and flushes when told that the utterance ends.  Everything else is the base class.

    v = ChunkedMBVocoder(generator, pqmf=None, slots=S, graph=True)     # pqmf: generator.pqmf (infer_hifigan.load_model)
    wav = v.step(mel, rows=None, last=None)   # (S, 1, Tc * hop + D * B): each slot's live samples in front, zeros behind
    v.counts                                  # samples emitted per slot by that step (host list; None with device counts)
    wav = v.flush(slot=None)                  # the held-back samples of one slot or of all: a step of no frames with `last`
    for wav in v.synthesize(mel_full, chunk_frames=8, slot=0): ...
    for index, wav in v.play_many(mels, chunk_frames=8): ...

``hop`` is the full ``prod(upsample_scales) * B``.  The chunks of an utterance add up to ``frames * hop`` samples: the first
is up to ``D * B`` samples shorter than its frames, the chunk that carries ``last`` that much longer.  ``hip.mb_emit`` is
the one host definition of the rule (the table is in include/kantts_hip.h).  After ``last`` the tail's own state of the slot
is as after a reset; the layers in front of it are not: ``reset(slot)`` before the slot takes another utterance, as
``play_many`` does.  ``synthesize`` and ``play_many`` are the base class's, on ``last`` from the utterance's frame cursor and
``mb_emitted``, the stateless form of the rule.

The emulated C ABI (oracle/cabi_numpy.py) has no entry point for the tail: the class says so at construction.
"""
import torch

import kantts._hip as hip
from kantts.models.hifigan.chunked import ChunkedVocoder, slot_ints

_NO_TAIL = ("the loaded C ABI has no multi-band tail (kantts_mb_tail_rows): ChunkedMBVocoder needs libkantts_hip.so, not the "
            "emulated ABI")


def mb_emitted(pos, n, T, low_hop, D, B):
    """(offset, count) of the samples a slot emits in the step that takes it from ``pos`` by ``n`` of its utterance's ``T``
    frames (``low_hop`` sub-band rows per frame, a look-ahead of ``D`` rows, ``B`` bands).  No running count is needed:
    after ``pos`` frames without ``last`` the synthesis holds back exactly min(pos * low_hop, D) rows, and ``last`` is set
    in the step that reaches T.  ``hip.mb_emit`` stays the rule."""
    e, _ = hip.mb_emit(min(pos * low_hop, D), n * low_hop, n > 0 and pos + n >= T, D)
    return 0, e * B


class ChunkedMBVocoder(ChunkedVocoder):
    """``ChunkedVocoder`` for causal generators with ``out_channels = B > 1`` followed by ``PQMF.synthesis``.

    Per slot it carries, beside the convolution state, ``hip.mb_state_words(D, B)`` words of the synthesis (one fp32 buffer
    (2, slots, words rounded up to 4), ping-pong with the arena: flipped, saved and restored with it).  ``conv_post`` and the
    synthesis are fp32 in both precision modes.

    Refused at construction, before anything is packed or launched: what the base refuses, single-band generators
    (``ChunkedVocoder`` plays them), NSF generators (multi-band NSF is not built), a missing ``pqmf``, ``pqmf.subbands !=
    out_channels``, shapes outside the kernel's contract (2 <= B <= 8, D <= 16, conv_post with k <= 11, dilation 1 and a
    multiple of 4 input channels in 4..512), and a library without the entry point."""

    _plays_multiband = True
    _end_kw, _solo = "last", True

    def __init__(self, generator, pqmf=None, slots=1, graph=True, max_graphs=8):
        g = generator
        if g.out_channels == 1:
            raise ValueError("ChunkedMBVocoder needs a multi-band generator (out_channels > 1); ChunkedVocoder plays the others")
        if g.nsf_enable:
            raise NotImplementedError("ChunkedMBVocoder: multi-band NSF generators are not supported")
        pq = pqmf if pqmf is not None else getattr(g, "pqmf", None)
        if pq is None:
            raise ValueError("ChunkedMBVocoder needs the generator's PQMF (pqmf=, or generator.pqmf as "
                             "infer_hifigan.load_model attaches it)")
        if int(pq.subbands) != int(g.out_channels):
            raise ValueError("ChunkedMBVocoder: the PQMF has %d sub-bands, the generator %d output channels"
                             % (int(pq.subbands), int(g.out_channels)))
        self._pq = pq
        super().__init__(g, slots=slots, graph=graph, max_graphs=max_graphs)
        dev = self.device
        self._poly = pq._poly_synthesis.detach().to(device=dev, dtype=torch.float32).contiguous().clone()
        self._state_ss = -(-hip.mb_state_words(self.D, self.B) // 4) * 4  # both halves start on a 16-byte boundary
        self._mb_state = torch.zeros(2, self.slots, self._state_ss, device=dev, dtype=torch.float32)
        self._last = torch.zeros(self.slots, device=dev, dtype=torch.int32)  # per-slot end-of-utterance flags of a step
        self.pending = [0] * self.slots  # low-rate rows held back per slot (host mirror; None once device counts were used)
        self.counts = None

    def _plan_extra(self, g):
        pq, L = self._pq, self.post
        self.B = int(g.out_channels)
        self.D = -int(pq.d_min)
        if tuple(pq._poly_synthesis.shape) != (self.B, self.B, 2 * self.D + 1):
            raise ValueError("ChunkedMBVocoder: polyphase weights %s, expected %s"
                             % (tuple(pq._poly_synthesis.shape), (self.B, self.B, 2 * self.D + 1)))
        if not (2 <= self.B <= hip.MB_MAX_B and 1 <= self.D <= hip.MB_MAX_D):
            raise NotImplementedError("ChunkedMBVocoder: %d sub-bands with a look-ahead of %d rows, kantts_mb_tail_rows takes "
                                      "2..%d sub-bands and at most %d rows" % (self.B, self.D, hip.MB_MAX_B, hip.MB_MAX_D))
        if not (L.N == self.B and 1 <= L.K <= hip.MB_MAX_K and L.step == 1 and L.Cin % 4 == 0 and 4 <= L.Cin <= 512):
            raise NotImplementedError(
                "ChunkedMBVocoder: conv_post (Cin %d, N %d, k %d, dilation %d) is outside what kantts_mb_tail_rows accepts "
                "(Cin a multiple of 4 in 4..512, k <= %d, dilation 1)" % (L.Cin, L.N, L.K, L.step, hip.MB_MAX_K))
        if not hip.mb_tail_entry_points():
            raise RuntimeError(_NO_TAIL)
        self.low_hop = self.hop  # rows of the sub-band signal per frame
        self.hop *= self.B

    # ------------------------------------------------------------------------------------------------------------
    def reset(self, slot=None):
        """Zero state for one slot (others untouched) or for all, the synthesis included: nothing is held back."""
        super().reset(slot)
        if slot is None:
            self._mb_state.zero_()
            self.pending = [0] * self.slots
        else:
            self._mb_state[:, int(slot)].zero_()
            if self.pending is not None:
                self.pending[int(slot)] = 0

    def _save_state(self):
        return (self.arena.clone(), self._mb_state.clone())

    def _restore_state(self, saved):
        self.arena.copy_(saved[0])
        self._mb_state.copy_(saved[1])

    def _tail(self, h, parity, rows, mul):
        """conv_post, tanh and the streamed synthesis in one launch: h (S, Tq, C) -> wav (S, 1, (Tq + D) * B)."""
        L = self.post
        S, Tq, _ = h.shape
        out = torch.empty((S, (Tq + self.D) * self.B), device=h.device, dtype=torch.float32)
        hin = hout = None
        if L.H:
            hin = self.arena[parity, 0, L.off:L.off + L.H * L.Cin]
            hout = self.arena[1 - parity, 0, L.off:L.off + L.H * L.Cin]
        ok = hip.mb_tail(h, hin, hout, L.w, self._poly, self._mb_state[parity, 0], self._mb_state[1 - parity, 0], out, S=S,
                         Tq=Tq, Cin=L.Cin, B=self.B, K=L.K, D=self.D, hist_ss=self.arena.shape[2], state_ss=self._state_ss,
                         bias=L.bias, rows=rows, row_mul=mul, last=self._last, in_leaky=L.in_leaky)
        if not ok:
            raise RuntimeError("kantts_mb_tail_rows declined the generator it was planned for")
        return out.view(S, 1, -1)

    def step(self, mel, rows=None, last=None):
        """mel (slots, C_mel, Tc), Tc >= 1 -> wav (slots, 1, Tc * hop + D * B): the samples every slot emits in front, 0.0
        behind.  ``rows`` as in ``ChunkedVocoder.step`` (None: every slot takes Tc frames).  ``last``: ``slots`` flags (a
        sequence, or an integer / bool tensor on the host or on the device), non-zero where the slot's utterance ends with
        this step: the slot then emits everything it held back (with ``rows[s] == 0``: a flush).  Afterwards ``counts`` is
        the host list of samples emitted per slot, ``hip.mb_emit`` on host-known ``rows`` and ``last``; with device tensors
        it is None (from then on, until ``reset()``) and the caller applies ``hip.mb_emit`` itself."""
        if mel.dim() != 3 or mel.shape[0] != self.slots or mel.shape[1] != self._step_channels or mel.shape[2] < 1:
            raise ValueError("mel must be (slots=%d, %d, Tc >= 1), got %s" % (self.slots, self._step_channels, tuple(mel.shape)))
        Tc = int(mel.shape[2])
        h_rows = [Tc] * self.slots if rows is None else slot_ints(rows, "rows", self.slots, bools=True)  # see slot_ints
        if torch.is_tensor(rows) and h_rows is not None:
            rows = h_rows
        h_last = [0] * self.slots if last is None else slot_ints(last, "last", self.slots, bools=True)
        if h_last is None:
            self._last.copy_(last.to(torch.int32))
        else:
            self._last.copy_(torch.tensor([int(bool(f)) for f in h_last], dtype=torch.int32))
        wav = super().step(mel, rows=rows)
        if h_rows is None or h_last is None or self.pending is None:
            self.pending = self.counts = None
        else:
            self.counts = []
            for s in range(self.slots):
                emitted, self.pending[s] = hip.mb_emit(self.pending[s], h_rows[s] * self.low_hop, h_last[s], self.D)
                self.counts.append(emitted * self.B)
        return wav

    def flush(self, slot=None):
        """The samples one slot (or every slot) still holds back: a step of no frames with ``last`` set there.  Returns the
        step's wav (slots, 1, hop + D * B); ``counts`` says how many samples of each slot are live."""
        if slot is not None and not 0 <= int(slot) < self.slots:
            raise IndexError("slot %r of %d" % (slot, self.slots))
        mel = torch.zeros(self.slots, self._step_channels, 1, device=self.device, dtype=torch.float32)
        flags = [int(slot is None or s == int(slot)) for s in range(self.slots)]
        return self.step(mel, rows=[0] * self.slots, last=flags)

    def _end_of(self, pos, n, T):
        return int(n > 0 and pos + n >= T)  # the end of an utterance: from its frame cursor

    def _emitted(self, pos, n, T):
        return mb_emitted(pos, n, T, self.low_hop, self.D, self.B)

    def _play_one(self, mel_full, T, n, slot):
        if self.pending is None:
            raise RuntimeError("ChunkedMBVocoder: the slots were advanced with device counts; reset() before synthesize")
        yield from super()._play_one(mel_full, T, n, slot)
