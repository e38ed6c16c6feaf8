"""SAM-BERT inference that hands out mel frames chunk by chunk (the acoustic half of streaming synthesis; the vocoder half
is kantts/models/hifigan/chunked.py).

``KanTtsSAMBERT.forward`` returns once the mel of the whole utterance exists.  The model does not need that: the token side
(text encoder, variance adaptor, length regulator) fixes the frame count before the first decoder step, the PNCA decoder
looks back over a band, every post-net memory block looks ahead ``rp`` frames only (3 of 41 taps with the shipped
``postnet_shift: 17``) and the post-net LSTM is unidirectional.  So a session keeps the FULL-LENGTH buffers of one-shot
inference -- the decoder's ``out`` and K | V cache, every FSMN layer's input and FIR input, the LSTM's ``gx`` / ``out`` /
``gates`` / ``c`` -- and advances them in step through the range entry points of the C ABI:

    kantts_pnca_decode_range     decoder steps [t, t + n) in one launch, resuming from ``out`` / ``xkv``
    kantts_fsmn_dwconv_fwd_rows  the rows of a memory block whose look-ahead has been decoded
    kantts_lstm_fwd_range        the recurrence over those rows, resuming from ``out`` / ``c_save``

Look-ahead arithmetic: with D frames decoded, the output of FSMN layer i is final up to D - sum_{j <= i} rp_j (up to the
end once D is the padded frame count: the FIR's zero padding past the end is in the kernel), everything behind the last
layer is position-wise or causal.  Shipped configuration: 4 layers x rp 3 = 12 frames behind the decoder.

    ca = ChunkedAcoustic(fsnet)
    sess = ca.open(inputs_ling, inputs_emotion, inputs_speaker, input_lengths)
    for lo, hi, mel in sess.stream(chunk_steps):     # mel (B, hi - lo, num_mels): FINAL post-net rows [lo, hi)
        ...
    res = sess.result()                              # the dictionary forward() returns

Sequences of a batch advance in lockstep, each with its own length and band width, as in batched one-shot inference.
Rows past a sequence's own frame count are padding; ``sess.live_rows(lo, hi)`` says how many of the rows [lo, hi) each
sequence really has, which is what a multi-slot vocoder takes as its per-slot counts:

    wav = vocoder.step(mel.transpose(1, 2), rows=sess.live_rows(lo, hi))     # every slot stops at its own last frame

Independently advancing slots (continuous batching) are kantts/models/sambert/slots.py.  Not here: graph capture of a step,
an fp32-mode decoder range.
"""
import torch
import torch.nn as nn

import kantts._hip as hip
from kantts._hip import ops
from kantts.models.sambert.ar_kernels import DecoderKernel
from kantts.models.utils import SeqInfo

_NO_RANGE = ("the loaded C ABI has no range entry points (kantts_pnca_decode_range, kantts_lstm_fwd_range, "
             "kantts_fsmn_dwconv_fwd_rows): chunked acoustic inference needs libkantts_hip.so, not the emulated ABI")


def _check(rc, what):
    if rc != 0:
        raise RuntimeError("libkantts_hip: %s failed with code %d" % (what, rc))


def live_rows(frames, lo, hi):
    """How many of the rows [lo, hi) exist in sequences of ``frames`` frames each: int32 clamp(frames - lo, 0, hi - lo)
    (pure; ``frames``: a tensor on any device, or a sequence of ints)."""
    return (torch.as_tensor(frames) - int(lo)).clamp(0, max(int(hi) - int(lo), 0)).to(torch.int32)


class ChunkedPostNet:
    """The post-net (FSMN -> LSTM -> Linear + residual) advanced over row ranges of full-length buffers.  Works in either
    precision mode; the position-wise contractions run through ``ops.linear`` on the row slices."""

    def __init__(self, postnet):
        lstm = postnet.lstm
        if lstm.num_layers != 1 or lstm.bidirectional or lstm.hidden_size != 128 or not lstm.batch_first:
            raise NotImplementedError("the streaming recurrence is one forward LSTM layer of 128 units")
        if postnet.training:
            raise ValueError("chunked inference needs eval() (dropout would draw per chunk)")
        for mb in postnet.fsmn.memory_block_lst:
            if mb.rp < 0 or mb.lp < 0:
                raise NotImplementedError("a memory block with a negative padding is not streamed")
        self.postnet = postnet
        self.lookahead = sum(mb.rp for mb in postnet.fsmn.memory_block_lst)

    @torch.no_grad()
    def open(self, x, lens64):
        """``x`` (B, T, num_mels): the full-length input buffer the caller fills row by row (rows at or after a sequence's
        length zero); ``lens64`` (B) frame counts."""
        if not hip.range_entry_points():
            raise RuntimeError(_NO_RANGE)
        return _PostNetRun(self, x, lens64)


class _PostNetRun:
    def __init__(self, cp, x, lens64):
        pn = cp.postnet
        B, T, _ = x.shape
        dev = x.device
        self.pn, self.B, self.T, self.x = pn, B, T, x
        info = SeqInfo(lens64, T)
        self.lens64, self.mask = info.lens64, info.mask
        U, H = pn.num_memory_units, pn.lstm_units

        def buf(*shape):
            return torch.empty(shape, device=dev, dtype=torch.float32)

        n = len(pn.fsmn.ffn_lst)
        self.ctx = [buf(B, T, U) for _ in range(n)]          # FIR input of layer i (its FFN's output)
        self.lay = [x] + [buf(B, T, U) for _ in range(n)]    # input of layer i; lay[n] feeds the LSTM
        self.gx, self.h = buf(B, T, 4 * H), buf(B, T, H)
        self.gates, self.cst = buf(1, B, T, 4 * H), buf(1, B, T, H)
        self.y = buf(B, T, pn.num_mels)
        self.whh = pn.lstm.weight_hh_l0.detach().contiguous().unsqueeze(0)
        self.bhh = pn.lstm.bias_hh_l0.detach().contiguous().unsqueeze(0)
        self.ffn_done = [0] * n   # rows of ctx[i] computed
        self.fir_done = [0] * n   # rows of lay[i + 1] final
        self.done = 0             # rows of y final

    @torch.no_grad()
    def advance(self, D):
        """Rows [0, D) of the input are final.  Returns (lo, hi): the rows of ``y`` that became final."""
        pn, T = self.pn, self.T
        avail = min(int(D), T)
        for i, (ffn, mb) in enumerate(zip(pn.fsmn.ffn_lst, pn.fsmn.memory_block_lst)):
            lo = self.ffn_done[i]
            if avail > lo:
                self.ctx[i][:, lo:avail] = ffn(self.lay[i][:, lo:avail].contiguous())
                self.ffn_done[i] = avail
            final = T if avail >= T else max(avail - mb.rp, 0)
            lo = self.fir_done[i]
            if final > lo:
                same = self.lay[i].size(-1) == pn.num_memory_units
                _check(hip.fsmn_dwconv_fwd_rows(self.ctx[i], mb.conv_dw.weight.detach().contiguous(), self.lay[i] if same else None,
                                                self.lens64, self.lay[i + 1], mb.lp, lo, final), "fsmn_dwconv_fwd_rows")
                self.fir_done[i] = final
            avail = self.fir_done[i]
        lo = self.done
        if avail > lo:
            lstm = pn.lstm
            self.gx[:, lo:avail] = ops.linear(self.lay[-1][:, lo:avail].contiguous(), lstm.weight_ih_l0, lstm.bias_ih_l0).float()
            _check(hip.lstm_fwd_range(self.gx, self.whh, self.bhh, None, self.h, self.gates, self.cst, lo, avail,
                                      1 if hip.get_precision() == "bf16" else 0), "lstm_fwd_range")
            self.y[:, lo:avail] = ops.linear(self.h[:, lo:avail].contiguous(), pn.fc.weight, pn.fc.bias,
                                             res=self.x[:, lo:avail].contiguous(),
                                             rowmask=self.mask[:, lo:avail].contiguous())
            self.done = avail
        return lo, self.done


class ChunkedAcoustic:
    """Streaming inference for one ``KanTtsSAMBERT``: needs eval(), bf16 mode and the decoder shapes
    ``DecoderKernel.eligible`` accepts (the one-launch decoder of csrc/ar_infer.hip); raises otherwise."""

    def __init__(self, fsnet):
        if fsnet.training:
            raise ValueError("chunked inference needs eval() (dropout would draw per chunk)")
        if hip.get_precision() != "bf16":
            raise ValueError("chunked acoustic inference runs the bf16-mode decoder kernel: set_precision('bf16') first")
        md = fsnet.mel_decoder
        if not DecoderKernel.eligible(md.mel_dec, md.d_mel, 0):
            raise NotImplementedError("the decoder's shapes are outside what the one-launch decoder kernel is compiled for")
        if not hip.range_entry_points():
            raise RuntimeError(_NO_RANGE)
        self.fsnet = fsnet
        self.postnet = ChunkedPostNet(fsnet.mel_postnet)
        self.lookahead = self.postnet.lookahead

    @torch.no_grad()
    def open(self, inputs_ling, inputs_emotion, inputs_speaker, input_lengths, duration_targets=None):
        return _AcousticSession(self, inputs_ling, inputs_emotion, inputs_speaker, input_lengths, duration_targets)


class _AcousticSession:
    def __init__(self, ca, inputs_ling, inputs_emotion, inputs_speaker, input_lengths, duration_targets):
        fsnet = ca.fsnet
        if fsnet.training or hip.get_precision() != "bf16":
            raise ValueError("a session needs eval() and bf16 mode")
        ts = fsnet._token_side(inputs_ling, inputs_emotion, inputs_speaker, input_lengths,
                               duration_targets=duration_targets)
        if ts.bw_int > 127:
            raise ValueError("band width %d: the decoder kernel holds bands up to 127" % ts.bw_int)
        md = fsnet.mel_decoder
        if md._decode_kernel is None:
            md._decode_kernel = DecoderKernel(md.mel_dec, md.d_mel)
        dk = md._decode_kernel
        dk.refresh()
        dec = md.mel_dec
        memory = ts.memory.contiguous().float()
        B, L = memory.size(0), memory.size(1)
        dev = memory.device
        self.ca, self.ts, self.dk = ca, ts, dk
        self.B, self.steps, self.r, self.d_mel = B, L, md.r, md.d_mel
        self.frames = ts.LR_length_rounded
        self.memory = memory
        self.hkv = ops.linear(memory, dk.hkv_w, dk.hkv_b).float().contiguous()
        self.xkv = torch.empty((len(dec.pnca), B, L, 256), device=dev, dtype=torch.float32)
        self.out = torch.empty((B, L, dec.dec_out_proj.out_features), device=dev, dtype=torch.float32)
        self.lens32 = ts.lfr_info.lens32.clamp(max=L)
        Tp = L * md.r
        self.Tp = Tp
        rows = ts.out_info.mask
        if rows.size(1) != Tp:
            rows = nn.functional.pad(rows, (0, Tp - rows.size(1)), value=True)
        self.rows = rows
        self.dec = torch.empty((B, Tp, md.d_mel), device=dev, dtype=torch.float32)  # masked decoder rows = post-net input
        self.post = ca.postnet.open(self.dec, ts.out_info.lens64)
        self.t = 0

    @property
    def finished(self):
        return self.t >= self.steps and self.post.done >= self.Tp

    @torch.no_grad()
    def step(self, n):
        """Advance every sequence by ``n`` decoder steps.  Returns (lo, hi, mel): mel (B, hi - lo, num_mels) are the FINAL
        post-net rows [lo, hi) -- hi = min(max(D - look-ahead, 0), padded frames) with D frames decoded, the padded frame
        count once the decoder has finished."""
        if n < 1:
            raise ValueError("step(n) needs n >= 1")
        if hip.get_precision() != "bf16":
            raise ValueError("a session needs bf16 mode")
        dec = self.ca.fsnet.mel_decoder.mel_dec
        t0, t1 = self.t, min(self.t + int(n), self.steps)
        if t1 > t0:
            _check(hip.pnca_decode_run(self.dk.w, self.dk.f, self.memory, self.hkv, self.xkv, self.out, self.lens32, self.ts.bw_dev,
                                       self.ts.bw_int, self.d_mel, len(dec.pnca), dec.d_model ** 0.5, dec.ln.eps,
                                       steps=(t0, t1)), "pnca_decode_range")
            lo, hi = t0 * self.r, t1 * self.r
            new = self.out[:, t0:t1].reshape(self.B, hi - lo, self.d_mel)
            self.dec[:, lo:hi] = new.masked_fill(self.rows[:, lo:hi].unsqueeze(-1), 0)
            self.t = t1
        lo, hi = self.post.advance(self.t * self.r)
        return lo, hi, self.post.y[:, lo:hi]

    def live_rows(self, lo, hi):
        """Per sequence, how many of the rows [lo, hi) of a chunk are frames of that sequence (int32, on the device)."""
        return live_rows(self.frames, lo, hi)

    def stream(self, chunk_steps):
        while not self.finished:
            yield self.step(chunk_steps)

    def result(self):
        """After the end: the dictionary ``forward`` returns (same keys, full tensors)."""
        if not self.finished:
            raise RuntimeError("result() before the last chunk: %d of %d decoder steps done" % (self.t, self.steps))
        return self.ca.fsnet._result(self.ts, None, self.dec, self.post.y, [], [])
