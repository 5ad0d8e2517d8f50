#!/usr/bin/env python3
"""Stand-in for the reference's generate_exp.py with its command line
(generate_exp.py [-l PATH] [-e PATH] [-m MODEL] [-a PATH] [-t PATH] RECIPE): speech /
non-speech scoring on the MI355X and decoding without AaltoASR; -a and -t are accepted and
ignored.  Parity with phone_probs and the token pass is unpinned
(speaker-diarization_amd/exp_generator.py).  --self-trained FCONFIG needs no model: the detector is
trained on each recording itself (speaker-diarization_amd/self_vad.py)."""
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
exp_generator = importlib.import_module('speaker-diarization_amd.exp_generator')

if __name__ == '__main__':
    sys.exit(exp_generator.main())
