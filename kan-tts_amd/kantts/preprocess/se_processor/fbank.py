"""Host side of kantts_kaldi_fbank: the constant tables of a Kaldi-compatible 80-bin log-mel front end at 16 kHz
(25 ms / 10 ms frames, povey window, 512-point FFT, Kaldi mel scale from 20 Hz to Nyquist), computed in fp64 once per
device, and the frame-count rule."""
import math

import torch

SAMPLE_RATE = 16000
WIN, HOP, N_FFT, N_MELS = 400, 160, 512, 80
LOW_FREQ = 20.0
_TABLES = {}


def num_frames(num_samples):
    """Frames of a waveform under Kaldi's snip_edges rule."""
    n = int(num_samples)
    return 0 if n < WIN else 1 + (n - WIN) // HOP


def _mel(f):
    return 1127.0 * math.log(1.0 + f / 700.0)


def mel_filters(n_mels=N_MELS, sample_rate=SAMPLE_RATE, n_fft=N_FFT, low=LOW_FREQ):
    """Kaldi's triangular filters (triangles in the MEL domain) as a dense (n_mels, n_fft / 2 + 1) fp64 tensor; the Nyquist
    bin gets no weight."""
    high = 0.5 * sample_rate
    m_lo, m_hi = _mel(low), _mel(high)
    delta = (m_hi - m_lo) / (n_mels + 1)
    bins = torch.zeros(n_mels, n_fft // 2 + 1, dtype=torch.float64)
    width = sample_rate / n_fft
    for m in range(n_mels):
        left, center, right = m_lo + m * delta, m_lo + (m + 1) * delta, m_lo + (m + 2) * delta
        for k in range(n_fft // 2):
            x = _mel(width * k)
            if left < x < right:
                bins[m, k] = (x - left) / (center - left) if x <= center else (right - x) / (right - center)
    return bins


def povey_window(n=WIN):
    i = torch.arange(n, dtype=torch.float64)
    return (0.5 - 0.5 * torch.cos(2.0 * math.pi * i / (n - 1))) ** 0.85


def kaldi_tables(device):
    """The tables kantts_kaldi_fbank reads (window, FFT twiddles, banded mel filters), on ``device``."""
    device = torch.device(device)
    if device not in _TABLES:
        dense = mel_filters()
        nz = dense > 0
        lo = nz.float().argmax(dim=1)
        cnt = nz.sum(dim=1)
        wmax = int(cnt.max())
        banded = torch.zeros(N_MELS, wmax, dtype=torch.float64)
        for m in range(N_MELS):
            banded[m, :int(cnt[m])] = dense[m, int(lo[m]):int(lo[m]) + int(cnt[m])]
        last = dense.shape[1] - 1 - nz.flip(1).float().argmax(dim=1)
        assert bool((last - lo + 1 == cnt).all())  # every filter is one contiguous band
        ang = 2.0 * math.pi * torch.arange(N_FFT // 2, dtype=torch.float64) / N_FFT
        _TABLES[device] = {
            "window": povey_window().float().to(device),
            "tw": torch.cat([torch.cos(ang), torch.sin(ang)]).float().to(device),
            "mel_lo": lo.to(torch.int32).to(device),
            "mel_n": cnt.to(torch.int32).to(device),
            "mel_w": banded.float().contiguous().to(device),
        }
    return _TABLES[device]
