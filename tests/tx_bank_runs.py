"""How the GPU modules of the transmit bank (tests/test_gpu_tx_bank.py, tests/test_gpu_tx_bank_limits.py) make their frames
and hold their outputs, one definition each: the device handle, a stream's own BERT frames, drawn frames of both parities,
the device buffer of output lanes with a canary in front of, between and behind them, the fill values and the error codes.
Needs no device to import."""
import numpy as np
import pytest

import tx_bank_model as M

FS = M.FRAME_SAMPLES                     # samples per frame; 2 int16 each
CANARY = 0x5A5B                          # int16 fill of everything a round must not touch
GAP = 32                                 # int16 per 64-byte canary
EINVAL, ECAPACITY, ESTATE = -1, -4, -6


@pytest.fixture(scope="module")
def dev():
    import torch
    return torch.device("cuda", 0)


def stream_frames(amd, k, n, first=0):
    """n BERT frames of stream k: its own callsign and token"""
    return amd.bert_frames(n, callsign=f"TXB{k}-{k}", token=0x10F0F0 + 0x010203 * k, first=first)


def drawn_frames(seed, n):
    """n frames of 134 drawn bytes. A frame's on-air parity is decided by its first byte (the last six bits the encoder sees:
    every earlier input bit reaches ten coded bits), and in a BERT frame that byte belongs to the callsign: all frames of one
    stream_frames stream have the same parity, so the sign parity it carries is its frame count's or 0
    (tests/test_tx_bank_host.py). Drawn frames mix both parities within an entry and from round to round."""
    return np.random.default_rng(seed).integers(0, 256, (n, 134), dtype=np.uint8)


class Lanes:
    """one device buffer of `lanes` outputs, back to back with a 64-byte canary in front of, between and behind them; everything
    starts as canary. `frames` is the number of frames of every lane, or a list of one count per lane (a lane of 0 frames is two
    canaries back to back)."""

    def __init__(self, dev, lanes, frames):
        import torch
        counts = [frames] * lanes if isinstance(frames, int) else list(frames)
        assert len(counts) == lanes
        if isinstance(frames, int):
            self.per = 2 * FS * frames                                       # (lanes of one size: the int16 of each)
        self.size = [2 * FS * n for n in counts]                             # int16 of each lane
        self.at = np.concatenate([[0], np.cumsum([s + GAP for s in self.size])]).astype(np.int64) + GAP   # where each starts; [-1]: the end
        self.buf = torch.full((int(self.at[-1]),), CANARY, dtype=torch.int16, device=dev)
        assert self.buf.data_ptr() % 64 == 0

    def ptr(self, lane, frame=0):
        return self.buf.data_ptr() + 2 * (int(self.at[lane]) + 2 * FS * frame)

    def lane(self, lane):
        a = int(self.at[lane])
        return self.buf[a:a + self.size[lane]].cpu().numpy()

    def canaries_intact(self):
        x = self.buf.cpu().numpy()
        return all((x[a - GAP:a] == CANARY).all() for a in self.at.tolist())
