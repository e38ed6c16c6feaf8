"""Symbols to waveform, chunk by chunk: the acoustic slot pool feeding the chunked vocoder on the device.

``AcousticSlots`` (kantts/models/sambert/slots.py) hands out FINAL post-net rows per slot; ``ChunkedVocoder.step(mel,
rows=...)`` / ``ChunkedNSFVocoder.step(feats, rows=...)`` / ``ChunkedMBVocoder.step(mel, rows=..., last=...)``
(kantts/models/hifigan) consume frames per slot.  ``StreamingTTS``
pairs acoustic slot ``s`` with vocoder slot ``s`` and joins them with one launch per step (csrc/handover.hip,
kantts_mel_handover_rows): the frames of every slot that are final but not yet vocoded go from the pool's channels-last
``y`` buffer into one channels-first (S, C, Tc) buffer -- for NSF voices with the f0 channel de-normalised and the voicing
channel binarised on the way, as ``infer_sambert.denorm_f0`` does on the host -- and that buffer is the vocoder's step
input.  No frame visits the host between the two halves.

    tts = StreamingTTS(fsnet, generator, slots=S, max_steps=L, chunk_frames=N, nsf=None | (scale, offset))
    for index, first_sample, wav in tts.play_many(requests, results=None): ...
    tts.admit(s, index, request); outs = tts.step(); tts.done(s); tts.release(s)

A step is one acoustic step (``chunk_frames / outputs_per_step`` decoder steps for every slot whose decoder has any left,
zero for the others) and then at most one vocoder step: slot ``s`` hands over ``min(chunk_frames, final_s - vocoded_s)``
frames, where ``final_s`` counts live frames only (the padding up to a multiple of ``outputs_per_step`` is never vocoded).
Its per-slot (start, count) pairs travel in ONE host-to-device copy, and a step in which no slot has a frame to hand over
launches no vocoder step.  A multi-band voice (``generator.out_channels > 1``) plays through ``ChunkedMBVocoder``, whose
synthesis bank holds back up to ``D * B`` samples per slot: the same copy then also carries a flag per slot, set in the step
that hands over the utterance's last frame, and that step emits everything held back -- so the audio of a step is what the
slot EMITTED (the vocoder's ``_emitted``), not ``n * hop`` samples, and ``first_sample`` is the running
sample count of the utterance.  The post-net's look-ahead delays the first frames of an utterance, so a slot is released only
after its last frame has been VOCODED: until then it takes zero-count acoustic steps while the vocoder drains what is left.

``lookahead=True`` lets a non-causal generator (single band) play, through ``ChunkedNCVocoder`` or, with a source module
(``nsf=``), through ``ChunkedNCNSFVocoder`` (kantts/models/hifigan/chunked_nc_nsf.py: the hand-over de-normalises f0 as for a
causal NSF voice, ``admit`` keys the utterance's excitation, flush frames are read by no launch): its audio
comes ``vocoder.delay_samples`` late, so the upload also carries every slot's frame count (``end``) and the vocoder's own
per-slot counts, which exceed the handed-over frames by flush frames once the acoustic frames have run out; the audio of a step
is what the slot emitted (``hip.nc_emit``), and a slot is released only after the flush.  ``step`` knows none of the
classes: it runs on the emission contract of ``ChunkedVocoder`` (flush frames, the end argument, the emitted run) with the
slot's vocoder at ``vocoded + flushed``, and ``kantts.models.hifigan.chunked_vocoder_class`` picks the class.  Without it such a generator is
refused as before: the added latency (``vocoder.flush_frames`` frames before the first sample) is a decision.

The emulated C ABI (oracle/cabi_numpy.py) has no hand-over entry point, as it has none of the per-slot ones: the class says
so at construction.

Not here: overlapping the acoustic step of chunk k + 1 with the vocoder step of chunk k on two streams, a captured acoustic
step.
"""
import torch

import kantts._hip as hip
from kantts.models.hifigan import chunked_vocoder_class
from kantts.models.sambert.slots import AcousticSlots

_NO_HANDOVER = ("the loaded C ABI has no hand-over entry point (kantts_mel_handover_rows): StreamingTTS needs "
                "libkantts_hip.so, not the emulated ABI")


class StreamingTTS:
    """``slots`` utterances at a time from linguistic inputs to audio through one ``KanTtsSAMBERT`` (eval, bf16 mode: the
    rules of ``AcousticSlots``) and one causal ``Generator`` (eval, on the same device: the rules of
    ``ChunkedVocoder`` / ``ChunkedNSFVocoder`` / ``ChunkedMBVocoder``, whichever the generator needs; a multi-band generator
    carries its ``pqmf``, as ``infer_hifigan.load_model`` attaches it).  ``max_steps``: decoder steps the buffers of a
    slot hold; ``chunk_frames``: frames per vocoder step, a positive multiple of ``outputs_per_step``; ``nsf=(scale,
    offset)``: the f0 de-normalisation of an NSF voice (mean_std: std and mean; global: max - min and min), with
    ``f0_threshold`` the floor in Hz and ``uv_threshold`` the voicing threshold; ``seed`` and ``graph`` go to the vocoder.

    Refused at construction, before anything is packed: a ``chunk_frames`` that is no positive multiple of
    ``outputs_per_step``, an acoustic model whose ``num_mels`` is not the generator's ``in_channels`` (+ 2 for NSF), an NSF
    generator without ``nsf=``, ``nsf=`` for a generator without a source module, a library without the hand-over entry
    point, and whatever either underlying class refuses."""

    def __init__(self, fsnet, generator, slots=1, max_steps=1024, chunk_frames=None, nsf=None, f0_threshold=30.0,
                 uv_threshold=0.6, seed=0, graph=True, lookahead=False):
        r = int(fsnet.mel_decoder.r)
        if chunk_frames is None or int(chunk_frames) < 1 or int(chunk_frames) % r:
            raise ValueError("chunk_frames must be a positive multiple of outputs_per_step (%d), got %r" % (r, chunk_frames))
        nsf_enable = bool(generator.nsf_enable)
        want = int(generator.conv_pre.conv1d.in_channels) + (2 if nsf_enable else 0)
        if int(fsnet.mel_postnet.num_mels) != want:
            raise ValueError("the acoustic model has num_mels = %d, the generator takes %d%s"
                             % (int(fsnet.mel_postnet.num_mels), want, " (mel bins + f0 + voicing)" if nsf_enable else ""))
        if nsf_enable and nsf is None:
            raise ValueError("an NSF generator needs nsf=(scale, offset), the f0 de-normalisation of its acoustic model")
        if nsf is not None and not nsf_enable:
            raise ValueError("nsf= was given for a generator without a source module")
        if not hip.handover_entry_points():
            raise RuntimeError(_NO_HANDOVER)
        self.nsf = None if nsf is None else (float(nsf[0]), float(nsf[1]))
        self.f0_threshold, self.uv_threshold = float(f0_threshold), float(uv_threshold)
        self.pool = AcousticSlots(fsnet, slots=slots, max_steps=max_steps)
        cls = chunked_vocoder_class(generator, lookahead)
        self.mb, self.nc = cls._plays_multiband, cls._plays_noncausal
        self.vocoder = cls(generator, slots=slots, graph=graph, **({"seed": seed} if cls._plays_nsf else {}))
        if self.vocoder.device != self.pool.dev:
            raise ValueError("the acoustic model is on %s, the generator on %s" % (self.pool.dev, self.vocoder.device))
        self.S, self.Tc, self.chunk_steps, self.hop = self.pool.S, int(chunk_frames), int(chunk_frames) // r, self.vocoder.hop
        self.buf = torch.zeros(self.S, want, self.Tc, device=self.pool.dev, dtype=torch.float32)  # the vocoder's step input
        # host cursors per slot: the request it plays (None: free), its live frames, how many are final, how many vocoded,
        # the samples emitted so far and (lookahead) the flush frames the vocoder has taken behind the utterance's last one
        self.index = [None] * self.S
        self.frames, self.final, self.vocoded = [0] * self.S, [0] * self.S, [0] * self.S
        self.samples, self.flushed = [0] * self.S, [0] * self.S
        self.flush_frames = self.vocoder.flush_frames

    # ------------------------------------------------------------------------------------------------ slots
    def admit(self, s, index, request):
        """Utterance ``index`` -- ``request``: the arguments of ``AcousticSlots.admit`` without the slot, a tuple or a
        dictionary -- into free slot ``s`` of both halves; the vocoder slot must be in its reset state (it is after
        construction and after ``release``).  ``index`` names the utterance to the vocoder: an NSF voice draws its noise
        and initial phases from (seed, index).  Returns the utterance's live frame count."""
        s = int(s)
        self.pool.admit(s, **request) if isinstance(request, dict) else self.pool.admit(s, *request)
        self.vocoder._assign(s, index)
        self.index[s] = index
        self.frames[s] = self.pool.live_rows(s, 0, self.pool.T)
        self.final[s] = self.vocoded[s] = self.samples[s] = self.flushed[s] = 0
        return self.frames[s]

    def done(self, s):
        """True once the last live frame of the slot's utterance has been vocoded (lookahead: and flushed out)."""
        s = int(s)
        if self.index[s] is None:
            raise ValueError("slot %d is free" % s)
        return self.pool.finished(s) and self.vocoded[s] >= self.frames[s] and self.flushed[s] >= self.flush_frames

    def release(self, s, results=None):
        """Free slot ``s`` of both halves after ``results[index] = pool.result(s)`` when a dictionary is given; the
        vocoder slot goes back to zero state."""
        s = int(s)
        if self.index[s] is None:
            raise ValueError("slot %d is free" % s)
        if results is not None:
            results[self.index[s]] = self.pool.result(s)
        self.pool.release(s)
        self.vocoder.reset(s)
        self.index[s] = None
        self.frames[s] = self.final[s] = self.vocoded[s] = self.samples[s] = self.flushed[s] = 0

    # ------------------------------------------------------------------------------------------------ step
    @torch.no_grad()
    def step(self):
        """One acoustic step, then at most one vocoder step.  Returns one entry per slot: None for a free slot, else
        ``(index, lo, n, wav)``: the slot's utterance, its frame position before this step, the frames handed over and
        their audio, (1, n * hop) (n may be 0: nothing of the slot was final yet, or everything has been vocoded).  A
        multi-band voice holds samples back: the audio is what the slot emitted, up to D * B samples fewer than n * hop, and
        that many more in the step that hands over the utterance's last frame.  With ``lookahead`` the audio is what the
        slot emitted too: nothing for the first ``flush_frames`` frames or so, and the rest in steps with n == 0 in which
        the vocoder takes flush frames."""
        pool, S, Tc = self.pool, self.S, self.Tc
        counts = [0] * S
        for s in range(S):
            if self.index[s] is not None:
                counts[s] = min(self.chunk_steps, pool.slot[s].steps - pool.slot[s].t)
        outs = pool.step(counts, capacity=self.chunk_steps)
        # the vocoder's side of the step, on the emission contract of ChunkedVocoder: slot s is at vocoded + flushed and
        # takes the frames handed over plus, once every live frame is final, flush frames behind the last one
        voc = self.vocoder
        rows, take, ends = [0] * S, [0] * S, [voc._end_of(0, 0, -1)] * S
        for s in range(S):
            if self.index[s] is not None:
                self.final[s] = max(self.final[s], min(outs[s][1], self.frames[s]))
                rows[s] = take[s] = min(Tc, self.final[s] - self.vocoded[s])
                if self.final[s] == self.frames[s]:
                    take[s] += min(Tc - rows[s], self.flush_frames - self.flushed[s])
                ends[s] = voc._end_of(self.vocoded[s] + self.flushed[s], take[s], self.frames[s])
        wav = None
        if any(take):
            A = torch.tensor([self.vocoded, rows, take] + ([ends] if voc._end_kw else []),
                             dtype=torch.int32).to(pool.dev, non_blocking=True)  # the ONE upload
            if any(rows):
                hip.check(hip.mel_handover(pool.y, A[0], A[1], self.buf, nsf=self.nsf, f0_floor=self.f0_threshold,
                                           uv_threshold=self.uv_threshold), "mel_handover_rows")
            wav = voc.step(self.buf, rows=A[2], **({voc._end_kw: A[3]} if voc._end_kw else {}))
        ret = [None] * S
        for s in range(S):
            if self.index[s] is not None:
                lo, n = self.vocoded[s], rows[s]
                off, m = voc._emitted(lo + self.flushed[s], take[s], self.frames[s])
                audio = wav[s, :, off:off + m] if m else torch.zeros(1, 0, device=pool.dev, dtype=torch.float32)
                ret[s] = (self.index[s], lo, n, audio)
                self.vocoded[s], self.flushed[s] = lo + n, self.flushed[s] + take[s] - n
        return ret

    def play_many(self, requests, results=None):
        """Continuous batching from symbols to audio: a generator that plays ``requests`` -- each the arguments of
        ``AcousticSlots.admit`` without the slot -- through all slots, yielding ``(index, first_sample, wav)`` with wav
        (1, n * hop) the next ``n`` frames of request ``index`` (a multi-band voice: the samples the step emitted, see
        ``step``; ``first_sample`` is the utterance's running sample count), in slot order after every step.  The schedule is that of
        the two halves' own ``play_many``: every slot must be free; the slots take requests in input order; a slot is
        released once its last frame has been vocoded -- after ``results[index] = pool.result(slot)`` when a dictionary is
        given -- and takes the next request before the next step.  The chunks of an utterance add up to frames * hop
        samples."""
        if any(i is not None for i in self.index) or len(self.pool.free_slots()) != self.S:
            raise ValueError("play_many needs every slot free")
        requests = list(requests)
        self.vocoder.reset()
        nxt = 0
        while True:
            for s in range(self.S):
                if self.index[s] is None and nxt < len(requests):
                    self.admit(s, nxt, requests[nxt])
                    nxt += 1
            if all(i is None for i in self.index):
                return
            for s, out in enumerate(self.step()):
                if out is not None and out[3].shape[-1] > 0:
                    yield out[0], self.samples[s], out[3]
                    self.samples[s] += int(out[3].shape[-1])
            for s in range(self.S):
                if self.index[s] is not None and self.done(s):
                    self.release(s, results)
