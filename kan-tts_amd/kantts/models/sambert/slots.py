"""A pool of SAM-BERT streaming slots that advance independently (continuous batching for the acoustic half; the vocoder
half is ``ChunkedVocoder.step(mel, rows=...)`` / ``play_many`` of kantts/models/hifigan/chunked.py).

``ChunkedAcoustic`` (chunked.py) plays one batch in lockstep: all sequences are admitted together, advance by the same
number of decoder steps, and the session lasts as long as its longest sequence.  Here ``S`` slots share fixed-capacity
buffers -- the full-length buffers of a ChunkedAcoustic session, allocated once at (S, max_steps, ...) and
(S, max_steps * r, ...) -- an utterance is admitted into a free slot at any time, and every ``step`` advances each slot by
its own count of decoder steps through the per-slot entry points of the C ABI:

    kantts_pnca_decode_slots       decoder steps [t0[s], t1[s]) of every slot in one launch
    kantts_fsmn_dwconv_fwd_slots   the rows of a memory block whose look-ahead has been decoded, per slot
    kantts_lstm_fwd_slots          the recurrence over those rows, per slot
    kantts_scatter_rows_f32        packed rows back into the full-length buffers (the inverse of kantts_ragged_rows_f32)

Look-ahead arithmetic, per slot: with D_s frames of slot s decoded, the output of FSMN layer i is final up to
D_s - sum_{j <= i} rp_j, or up to the utterance's own padded frame count steps_s * r once its decoder has finished;
everything behind the last layer is position-wise or causal.  The cursors (decoder steps done, rows of every FFN / FIR
output, rows of the result) live on the host, so a step's whole schedule is known before its first launch: all per-slot
(start, count) arrays of the step travel in ONE host-to-device copy, and a stage whose windows are all empty is not
launched (a step whose counts are all zero launches nothing).

The position-wise contractions (FSMN feed-forwards, LSTM input projection, final Linear + residual + row mask) have ragged
row windows: each gathers its slots' new rows into a packed (S, Tcap, C) buffer (kantts_ragged_rows_f32), runs the model's
own ``ops.linear`` on it and puts the rows back (kantts_scatter_rows_f32).  Tcap = min(capacity * r + look-ahead,
max_steps * r) depends on the step's capacity only, so the shapes of a ``play_many`` run are static.

    pool = AcousticSlots(fsnet, slots=S, max_steps=Lmax)
    frames = pool.admit(s, inputs_ling, inputs_emotion, inputs_speaker, input_lengths)   # ONE utterance into free slot s
    outs = pool.step(counts)          # outs[s]: None (free slot) or (lo, hi, mel): FINAL post-net rows [lo, hi) of slot s
    pool.finished(s); pool.result(s); pool.release(s); pool.free_slots()
    for index, lo, hi, mel in pool.play_many(requests, chunk_steps): ...

Not here: graph capture of a step, an fp32-mode decoder range.
"""
import torch

import kantts._hip as hip
from kantts._hip import ops
from kantts.models.sambert.ar_kernels import DecoderKernel
from kantts.models.sambert.chunked import ChunkedPostNet, _check

_NO_SLOTS = ("the loaded C ABI has no per-slot entry points (kantts_pnca_decode_slots, kantts_lstm_fwd_slots, "
             "kantts_fsmn_dwconv_fwd_slots, kantts_scatter_rows_f32): acoustic slots need libkantts_hip.so, not the emulated ABI")


class _Slot:
    """Host-side state of one occupied slot."""

    __slots__ = ("ts", "steps", "frames", "Tp", "t", "ffn_done", "fir_done", "done")

    def __init__(self, ts, steps, frames, r, n_layers):
        self.ts, self.steps, self.frames, self.Tp = ts, steps, frames, steps * r
        self.t = 0                       # decoder steps done
        self.ffn_done = [0] * n_layers   # rows of ctx[i] computed
        self.fir_done = [0] * n_layers   # rows of lay[i + 1] final
        self.done = 0                    # rows of y final


class AcousticSlots:
    """``slots`` independently advancing streaming sessions of one ``KanTtsSAMBERT`` over buffers of ``max_steps`` decoder
    steps each: needs eval(), bf16 mode and the decoder shapes ``DecoderKernel.eligible`` accepts (the rules of
    ChunkedAcoustic); raises otherwise.  The buffers are sized in decoder steps: for a filled-pause (FP) model the
    inserted filler rows lengthen an utterance, and one that no longer fits is refused at ``admit`` like any other."""

    def __init__(self, fsnet, slots, max_steps):
        if fsnet.training:
            raise ValueError("acoustic slots need eval() (dropout would draw per chunk)")
        if hip.get_precision() != "bf16":
            raise ValueError("acoustic slots run the bf16-mode decoder kernel: set_precision('bf16') first")
        md = fsnet.mel_decoder
        if not DecoderKernel.eligible(md.mel_dec, md.d_mel, 0):
            raise NotImplementedError("the decoder's shapes are outside what the one-launch decoder kernel is compiled for")
        if not (hip.range_entry_points() and hip.slot_entry_points()):
            raise RuntimeError(_NO_SLOTS)
        S, L = int(slots), int(max_steps)
        if S < 1 or L < 1:
            raise ValueError("slots and max_steps must be >= 1")
        self.fsnet, self.S, self.L = fsnet, S, L
        pn = fsnet.mel_postnet
        self.pn = pn
        self.lookahead = ChunkedPostNet(pn).lookahead   # also refuses a post-net that cannot be streamed
        self.r, self.d_mel = md.r, md.d_mel
        self.T = T = L * md.r
        dev = next(fsnet.parameters()).device
        self.dev = dev
        dec = md.mel_dec

        def buf(*shape):
            return torch.zeros(shape, device=dev, dtype=torch.float32)

        # decoder side: the buffers of _AcousticSession at (S, L, ...)
        self.memory = None  # (S, L, d_mem): allocated by the first admit, which knows d_mem
        self.hkv = buf(S, L, len(dec.pnca) * 256)
        self.xkv = buf(len(dec.pnca), S, L, 256)
        self.out = buf(S, L, dec.dec_out_proj.out_features)
        self.lens32 = torch.zeros(S, device=dev, dtype=torch.int32)   # decoder steps of the slot's utterance (0: free)
        self.lens64 = torch.zeros(S, device=dev, dtype=torch.int64)   # its frame count
        self.bw = torch.zeros(S, device=dev, dtype=torch.int32)       # its band width (always the per-sequence device form)
        # post-net side: the buffers of _PostNetRun at (S, T, ...)
        U, H = pn.num_memory_units, pn.lstm_units
        n = len(pn.fsmn.ffn_lst)
        self.dec = buf(S, T, md.d_mel)                               # masked decoder rows = post-net input
        self.ctx = [buf(S, T, U) for _ in range(n)]                   # FIR input of layer i (its FFN's output)
        self.lay = [self.dec] + [buf(S, T, U) for _ in range(n)]      # input of layer i; lay[n] feeds the LSTM
        self.gx, self.h = buf(S, T, 4 * H), buf(S, T, H)
        self.gates, self.cst = buf(1, S, T, 4 * H), buf(1, S, T, H)
        self.y = buf(S, T, pn.num_mels)
        self.whh = pn.lstm.weight_hh_l0.detach().contiguous().unsqueeze(0)
        self.bhh = pn.lstm.bias_hh_l0.detach().contiguous().unsqueeze(0)
        self.row_off = torch.arange(S, device=dev, dtype=torch.int64) * T   # first row of slot s in a flat (S * T, C) view
        self.slot = [None] * S

    # ------------------------------------------------------------------------------------------------ bookkeeping
    def free_slots(self):
        return [s for s in range(self.S) if self.slot[s] is None]

    def _occupied(self, s):
        st = self.slot[int(s)]
        if st is None:
            raise ValueError("slot %d is free" % int(s))
        return st

    def finished(self, s):
        """True once the slot's decoder has run all its steps and its post-net has flushed."""
        st = self._occupied(s)
        return st.t >= st.steps and st.done >= st.Tp

    def release(self, s):
        """Free the slot.  Nothing is cleared: the next occupant overwrites what it reads."""
        self._occupied(s)
        s = int(s)
        self.slot[s] = None
        self.lens32[s] = 0
        self.lens64[s] = 0

    def live_rows(self, s, lo, hi):
        """How many of the rows [lo, hi) of slot ``s`` are frames of its utterance (host int): a vocoder slot's ``rows``."""
        st = self._occupied(s)
        return min(max(st.frames - int(lo), 0), max(int(hi) - int(lo), 0))

    # ------------------------------------------------------------------------------------------------ admit
    @torch.no_grad()
    def admit(self, s, inputs_ling, inputs_emotion, inputs_speaker, input_lengths, duration_targets=None):
        """ONE utterance (batch 1) into free slot ``s``: the token side and the memory K | V projection run exactly as
        ``forward`` at batch 1 runs them.  Returns the utterance's frame count."""
        s = int(s)
        if not 0 <= s < self.S:
            raise ValueError("slot %d of %d" % (s, self.S))
        if self.slot[s] is not None:
            raise ValueError("slot %d is occupied" % s)
        fsnet = self.fsnet
        if fsnet.training or hip.get_precision() != "bf16":
            raise ValueError("acoustic slots need eval() and bf16 mode")
        if inputs_ling.size(0) != 1:
            raise ValueError("admit takes one utterance (batch 1), got a batch of %d" % inputs_ling.size(0))
        ts = fsnet._token_side(inputs_ling, inputs_emotion, inputs_speaker, input_lengths, duration_targets=duration_targets)
        if ts.bw_int > 127:
            raise ValueError("band width %d: the decoder kernel holds bands up to 127" % ts.bw_int)
        md = fsnet.mel_decoder
        if md._decode_kernel is None:
            md._decode_kernel = DecoderKernel(md.mel_dec, md.d_mel)
        dk = md._decode_kernel
        dk.refresh()
        self.dk = dk
        memory = ts.memory.contiguous().float()
        steps = int(memory.size(1))
        if steps > self.L:
            fp = (" (%d token rows after the filled-pause insertion)" % int(ts.inter_lengths.reshape(-1)[0])
                  if getattr(fsnet, "fp_enable", False) else "")
            raise ValueError("the utterance has %d decoder steps%s, the pool's buffers hold max_steps = %d" % (steps, fp, self.L))
        hkv = ops.linear(memory, dk.hkv_w, dk.hkv_b).float().contiguous()
        if self.memory is None:
            self.memory = torch.zeros((self.S, self.L, memory.size(2)), device=self.dev, dtype=torch.float32)
        self.memory[s, :steps] = memory[0]
        self.hkv[s, :steps] = hkv[0]
        self.lens32[s] = ts.lfr_info.lens32.clamp(max=steps)[0]
        self.lens64[s] = ts.out_info.lens64[0]
        self.bw[s] = ts.bw_dev.reshape(-1)[0]
        frames = int(ts.LR_length_rounded[0])
        self.slot[s] = _Slot(ts, steps, min(frames, steps * self.r), self.r, len(self.ctx))
        return frames

    # ------------------------------------------------------------------------------------------------ step
    def _plan(self, counts):
        """The step's whole schedule from the host-side cursors: a list of int32 rows of S entries each (uploaded in one
        copy) and, per stage, the index of its rows -- or None when every window of the stage is empty."""
        S, r = self.S, self.r
        rows = []

        def add(*rws):
            rows.extend(rws)
            return len(rows) - len(rws)

        t0 = [st.t if st else 0 for st in self.slot]
        t1 = [min(st.t + int(c), st.steps) if st else 0 for st, c in zip(self.slot, counts)]
        plan = {"dec": None, "ffn": [], "fir": [], "lstm": None}
        if any(b > a for a, b in zip(t0, t1)):
            lo = [a * r for a in t0]
            n = [(b - a) * r for a, b in zip(t0, t1)]
            live = [min(max(st.frames - l, 0), k) if st else 0 for st, l, k in zip(self.slot, lo, n)]
            plan["dec"] = add(t0, t1, lo, n, live)
        avail = [b * r if st else 0 for st, b in zip(self.slot, t1)]
        for i, mb in enumerate(self.pn.fsmn.memory_block_lst):
            lo = [st.ffn_done[i] if st else 0 for st in self.slot]
            n = [max(a - l, 0) for a, l in zip(avail, lo)]
            plan["ffn"].append(add(lo, n) if any(n) else None)
            f0 = [st.fir_done[i] if st else 0 for st in self.slot]
            final = [((st.Tp if a >= st.Tp else max(a - mb.rp, 0)) if st else 0) for st, a in zip(self.slot, avail)]
            f1 = [max(f, l) for f, l in zip(final, f0)]
            plan["fir"].append(add(f0, f1) if any(b > a for a, b in zip(f0, f1)) else None)
            for st, a, b in zip(self.slot, avail, f1):
                if st:
                    st.ffn_done[i] = max(st.ffn_done[i], a)
                    st.fir_done[i] = b
            avail = f1
        lo = [st.done if st else 0 for st in self.slot]
        n = [max(a - l, 0) for a, l in zip(avail, lo)]
        if any(n):
            plan["lstm"] = add(lo, [l + k for l, k in zip(lo, n)], n)
        ret = []
        for st, b, l, k in zip(self.slot, t1, lo, n):
            if st:
                st.t, st.done = b, l + k
            ret.append((l, l + k) if st else None)
        return rows, plan, ret

    def _packed(self, src, A, lo, n, Tcap, lens=None):
        """Rows [lo[s], lo[s] + n[s]) of every slot of ``src`` (S, T, C) as a packed (S, Tcap, C) tensor, zero behind."""
        return hip.ragged_rows(src.view(self.S * self.T, src.size(-1)), self.row_off, A[n] if lens is None else lens, Tcap,
                               start=A[lo])

    def _put(self, packed, dst, A, lo, n):
        _check(hip.scatter_rows(packed.float().contiguous(), self.row_off, A[n], dst.view(self.S * self.T, dst.size(-1)),
                                start=A[lo]), "scatter_rows_f32")

    @torch.no_grad()
    def step(self, counts, capacity=None):
        """Advance slot s by ``counts[s]`` decoder steps (>= 0; what the utterance has left if that is fewer; ignored for a
        free slot) and its post-net as far as its own look-ahead allows.  ``capacity``: the largest count this pool is
        stepped with (default: the largest of ``counts``); it sizes the packed buffers of the contractions.  Returns a list:
        None for a free slot, else (lo, hi, mel) with mel (hi - lo, num_mels) the FINAL post-net rows [lo, hi) of the slot
        (a view of the pool's buffer: valid until the slot is released and reused)."""
        counts = [int(c) for c in counts]
        if len(counts) != self.S or min(counts) < 0:
            raise ValueError("step takes %d counts >= 0, got %s" % (self.S, counts))
        if hip.get_precision() != "bf16":
            raise ValueError("acoustic slots need bf16 mode")
        cap = max(counts) if capacity is None else int(capacity)
        if cap < max(counts):
            raise ValueError("capacity %d is below the largest count %d" % (cap, max(counts)))
        rows, plan, ret = self._plan(counts)
        if rows:
            pn, dec = self.pn, self.fsnet.mel_decoder.mel_dec
            Tcap = min(cap * self.r + self.lookahead, self.T)
            A = torch.tensor(rows, dtype=torch.int32).to(self.dev, non_blocking=True)   # the step's ONE upload
            k = plan["dec"]
            if k is not None:
                _check(hip.pnca_decode_run(self.dk.w, self.dk.f, self.memory, self.hkv, self.xkv, self.out, self.lens32, self.bw,
                                           0, self.d_mel, len(dec.pnca), dec.d_model ** 0.5, dec.ln.eps,
                                           slots=(A[k], A[k + 1])), "pnca_decode_slots")
                # the new decoder rows, zero at and after the slot's frame count, become post-net input
                new = self._packed(self.out.view(self.S, self.T, self.d_mel), A, k + 2, k + 3, Tcap, lens=A[k + 4])
                self._put(new, self.dec, A, k + 2, k + 3)
            for i, (ffn, mb) in enumerate(zip(pn.fsmn.ffn_lst, pn.fsmn.memory_block_lst)):
                k = plan["ffn"][i]
                if k is not None:
                    self._put(ffn(self._packed(self.lay[i], A, k, k + 1, Tcap)), self.ctx[i], A, k, k + 1)
                k = plan["fir"][i]
                if k is not None:
                    same = self.lay[i].size(-1) == pn.num_memory_units
                    _check(hip.fsmn_dwconv_fwd_slots(self.ctx[i], mb.conv_dw.weight.detach().contiguous(),
                                                     self.lay[i] if same else None, self.lens64, self.lay[i + 1], mb.lp,
                                                     A[k], A[k + 1], Tcap), "fsmn_dwconv_fwd_slots")
            k = plan["lstm"]
            if k is not None:
                lstm = pn.lstm
                gx = ops.linear(self._packed(self.lay[-1], A, k, k + 2, Tcap), lstm.weight_ih_l0, lstm.bias_ih_l0)
                self._put(gx, self.gx, A, k, k + 2)
                _check(hip.lstm_fwd_slots(self.gx, self.whh, self.bhh, None, self.h, self.gates, self.cst, A[k], A[k + 1],
                                          1), "lstm_fwd_slots")
                # rows at or after the slot's frame count are zeroed by the contraction's row mask
                pos = A[k].to(torch.int64)[:, None] + torch.arange(Tcap, device=self.dev)[None, :]
                mask = pos >= self.lens64[:, None]
                y = ops.linear(self._packed(self.h, A, k, k + 2, Tcap), pn.fc.weight, pn.fc.bias,
                               res=self._packed(self.dec, A, k, k + 2, Tcap), rowmask=mask.contiguous())
                self._put(y, self.y, A, k, k + 2)
        return [None if w is None else (w[0], w[1], self.y[s, w[0]:w[1]]) for s, w in enumerate(ret)]

    # ------------------------------------------------------------------------------------------------ results
    def result(self, s):
        """After the slot's last chunk: the dictionary ``forward`` returns for that utterance at batch 1 (same keys; the
        frame tensors are copies trimmed to the utterance's own padded length)."""
        st = self._occupied(s)
        if not self.finished(s):
            raise RuntimeError("result() before the last chunk: %d of %d decoder steps done" % (st.t, st.steps))
        s = int(s)
        return self.fsnet._result(st.ts, None, self.dec[s:s + 1, :st.Tp].clone(), self.y[s:s + 1, :st.Tp].clone(), [], [])

    def play_many(self, requests, chunk_steps, results=None):
        """Continuous batching: a generator that plays ``requests`` -- each the arguments of ``admit`` without the slot, as a
        tuple or a dictionary -- through all slots, yielding ``(index, lo, hi, mel)`` with mel (hi - lo, num_mels) the FINAL
        post-net rows [lo, hi) request ``index`` advanced by (only when hi > lo).  The schedule (that of
        ``ChunkedVocoder.play_many``): every slot must be free; the slots take requests in input order; every step gives
        each live slot ``chunk_steps`` decoder steps, or what it has left; a slot whose decoder has finished takes
        zero-count steps until its post-net has flushed; a slot whose post-net has flushed is released -- after
        ``results[index] = result(slot)`` when a dictionary ``results`` is given -- and takes the next request before the
        next step."""
        n = int(chunk_steps)
        if n < 1:
            raise ValueError("chunk_steps must be >= 1")
        if len(self.free_slots()) != self.S:
            raise ValueError("play_many needs every slot free")
        requests = list(requests)
        cur, nxt = [None] * self.S, 0
        while True:
            for s in range(self.S):
                if cur[s] is None and nxt < len(requests):
                    req = requests[nxt]
                    self.admit(s, **req) if isinstance(req, dict) else self.admit(s, *req)
                    cur[s], nxt = nxt, nxt + 1
            if all(c is None for c in cur):
                return
            counts = [0 if c is None else min(n, self.slot[s].steps - self.slot[s].t) for s, c in enumerate(cur)]
            outs = self.step(counts, capacity=n)
            for s, c in enumerate(cur):
                if c is not None and outs[s][1] > outs[s][0]:
                    yield (c,) + outs[s]
            for s, c in enumerate(cur):
                if c is not None and self.finished(s):
                    if results is not None:
                        results[c] = self.result(s)
                    self.release(s)
                    cur[s] = None
