#!/usr/bin/env python3
"""Writes tests/golden/vad_model.json: the STRUCTURE of the reference's speech / non-speech
model (hmms/mfcc_16g_11.10.2007_10.{cfg,gk,mc,ph}, vad_models/sp_nsp.lex, vad_models/malli.bin)
as read by speaker-diarization_amd/vad_model.py -- kernel count and dimension, the kernel
indices of every state, the word loop, the feature configuration's parameters -- and SHA-256
sums of its trained numbers (means, variances, weights, transition and LM probabilities, the
.cfg arrays), which are model data and are NOT stored.  Runs where the reference tree is at
hand (SPKD_REFERENCE); the tests write synthetic models of the same structure.

    python tests/golden/make_golden_vad_model.py
"""
import importlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
REF = os.environ.get('SPKD_REFERENCE', '/root/reference')
MODEL = 'hmms/mfcc_16g_11.10.2007_10'


def main():
    vm = importlib.import_module('speaker-diarization_amd.vad_model')
    from vad_numpy import model_structure
    old = os.getcwd()
    os.chdir(REF)                    # the lexicon and LM resolve against the working directory
    try:
        model = vm.VadModel.load(MODEL)
    finally:
        os.chdir(old)
    doc = dict(model_structure(model), model=MODEL,
               source="parsed from the reference's VAD model files by speaker-diarization_amd/vad_model.py "
                      "(tests/golden/make_golden_vad_model.py); trained numbers as SHA-256 only")
    with open(os.path.join(HERE, 'vad_model.json'), 'w') as f:
        json.dump(doc, f, indent=1)


if __name__ == '__main__':
    main()
