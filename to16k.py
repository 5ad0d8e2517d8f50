#!/usr/bin/env python3
"""Resample and downmix one 16-bit PCM .wav to 16 kHz mono on the MI355X: the step the reference
leaves to `ffmpeg -i x -ar 16000 -ac 1` (spk-diarization2.py:83), for .wav input of any rate and
channel count.  ./to16k.py IN.wav [-o OUT.wav] [-r 16000] [--beamform].  Parity with ffmpeg's
resampler is unpinned (speaker-diarization_amd/frontend.py, resample_taps).  --beamform aligns the
channels of a microphone array by their GCC-PHAT delays before summing them, instead of averaging
them (frontend.BEAMFORM; parity with any other beamformer is unpinned)."""
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
frontend = importlib.import_module('speaker-diarization_amd.frontend')

if __name__ == '__main__':
    sys.exit(frontend.to16k_main())
