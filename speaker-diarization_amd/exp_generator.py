"""Stand-in for the reference's generate_exp.py (stage 1 of spk-diarization2.py): per `audio=`
line of a recipe, speech / non-speech state scores into `<lnapath>/<base>.lna`, the decision
border shift, `<exppath>/<base>.last_frame` and the decoded token stream `<exppath>/<base>.exp`.

  features  the model's .cfg through spkd_mfcc (frontend.extract_device; 256-sample windows
            for the shipped VAD models), left on the device; a batch through spkd_mfcc_batch
  scores    spkd_gmm_loglik: natural-log state likelihoods of the .gk / .mc mixtures
            (what AaltoASR's phone_probs writes, generate_exp.py:94-97)
  .lna      phone_probs's layout: 4 header bytes (the state count), one byte 4, float32
            scores frame-major
  shift     shift_dec_bord exactly as generate_exp.py:177-186 computes it, float64 numpy in the
            same order -- including its quirk: the frame-major data is reshaped to
            (n_models, -1), so each value is normalised against one from the other half of
            the file, not against the other state of its frame
  decoder   spkd_vad_viterbi: an exact Viterbi over the word loop of sp_nsp.lex in place of
            AaltoASR's token pass (generate_exp.py:189-239), transition scale 2, LM scale 10,
            insertion penalty 1, no sentence end required
  .exp      "<first frame> <word>" per word of the best path, single spaces, no newline
            (_clean_decoder_output, generate_exp.py:134-137)

  --self-trained FCONFIG   no model at all: the detector is trained on each recording itself over the
            features of that configuration file (self_vad.py); .exp and .last_frame as ever, no .lna

PARITY UNPINNED where AaltoASR computes (front-end, likelihood convention, decoder): each
choice is listed in INTEGRATION.md and restated in the test suite's numpy file.  The .lna
layout, the shift, .last_frame and the file naming are the reference's own.
"""
import argparse
import os
import os.path as op
import re

import numpy as np

from . import feaconfig, frontend, hipabi, self_vad
from .vad_model import VadModel

SHIFT_BORD = 0.2
LNA_BYTES = 4


def get_lnas(recipe, lnapath):
    """[(wav, lna path)] per non-empty recipe line, as generate_exp.py:100-110 finds them
    (a line without audio= fails there the same way)."""
    audio_file = re.compile(r'audio=(\S+)')
    out = []
    with open(recipe) as rec:
        for line in rec:
            if line != '\n':
                wav = audio_file.search(line).groups()[0]
                out.append((wav, op.join(lnapath, op.splitext(op.basename(wav))[0] + '.lna')))
    return out


def lna_header(n_models):
    """The 4 count bytes, most significant first (generate_exp.py:121-124 reads them back)."""
    return bytes([(n_models >> 24) & 255, (n_models >> 16) & 255, (n_models >> 8) & 255, n_models & 255])


def write_scores_lna(path, scores):
    """The .lna phone_probs leaves: header, bytes per value (4), float32 [T][S] frame-major."""
    scores = np.ascontiguousarray(scores, dtype='<f4')
    with open(path, 'wb') as f:
        f.write(lna_header(scores.shape[1]))
        f.write(bytes([LNA_BYTES]))
        f.write(scores.tobytes())


def read_lna(lna):
    """generate_exp.py:119-129 (_read_lna)."""
    with open(lna, 'rb') as f:
        num_models = np.fromfile(f, np.uint8, count=4)
        dim = np.sum(num_models * np.array([16777216, 4096, 256, 1]))
        num_bytes = np.fromfile(f, np.int8, count=1)[0]
        dtype = np.float32 if num_bytes == 4 else np.int16
        return num_models, np.fromfile(f, dtype).reshape((dim, -1)).astype(np.float64)


def write_lna(lna, num_models, data, exppath):
    """generate_exp.py:132-142 (_write_lna): the .lna and <exppath>/<base>.last_frame."""
    with open(lna, 'wb') as f:
        num_models.tofile(f)
        np.array([4], dtype=np.int8).tofile(f)
        data.astype(np.float32).tofile(f)
    last_frame = '%d' % data.shape[1]
    with open(op.join(exppath, op.splitext(op.basename(lna))[0] + '.last_frame'), 'w') as f:
        f.write(last_frame)


def shift_dec_bord(lna, exppath):
    """generate_exp.py:177-186 for one file, in the same float64 operations and order."""
    num_models, l = read_lna(lna)
    with np.errstate(all='ignore'):
        l = np.exp(l)
        l[1, :] *= SHIFT_BORD
        l /= sum(l)
        l = np.log(l)
    write_lna(lna, num_models, l, exppath)


def lna_scores(lna):
    """The frame-major [T, S] float32 scores of an .lna, as the decoder reads them."""
    with open(lna, 'rb') as f:
        raw = f.read()
    n = int(sum(b * m for b, m in zip(raw[:4], (16777216, 4096, 256, 1))))
    return np.frombuffer(raw[5:], dtype='<f4').reshape(-1, n)


def exp_text(model, scores):
    """The .exp token stream of one file's (shifted) scores."""
    stay, exit_, enter = model.decoder_constants()
    frames, words, _ = hipabi.vad_viterbi(scores, model.word_state, stay, exit_, enter)
    return ' '.join('%d %s' % (t, model.words[w]) for t, w in zip(frames, words))


def device_scores(ctx, model, pcm):
    """float32 [T, S] state scores of int16 samples: features and scores on the device, the
    scores alone come back."""
    d_feat, T = frontend.extract_device(pcm, model.cfg, ctx)
    out = np.zeros((T, model.n_states), dtype=np.float32)
    if T == 0:
        return out
    d_sc = None
    try:
        d_sc = ctx.dev_alloc(out.nbytes)
        ctx.gmm_loglik(d_feat, T, model.gmm_arrays(), d_sc)
        ctx.d2h(out, d_sc)
    finally:
        ctx.dev_free(d_feat)
        ctx.dev_free(d_sc)
    return out


def decode_batch(ctx, model, pcms, timings=None, uploaded=None):
    """The decision part of stage 1 for a batch of files, on the device: per file of int16 samples
    the .exp token list [(first frame, word name)] and the .last_frame value.  One upload of the
    samples (or `uploaded`, the (d_pcm, sample_off) pair of a frontend.upload_batch the caller
    shares with another chain; pcms is not read then; upload_batch takes integer samples that fit
    int16 and refuses the rest with ValueError), the front-end once for every file
    (frontend.extract_batch: the borders are each file's own), spkd_gmm_loglik once on the
    concatenation, the border shift (in place) and the decoding one call each
    (spkd_vad_shift_batch, spkd_vad_viterbi_batch); the scores never come to the host.
    Returns (tokens, last_frames)."""
    d_pcm, sample_off = uploaded if uploaded is not None else frontend.upload_batch(ctx, pcms, timings)
    d_feat, off = frontend.extract_batch(ctx, model.cfg, d_pcm, sample_off, timings=timings)
    last_frames = [int(n) for n in np.diff(off)]
    total = int(off[-1])
    d_sc = ctx.dev_scratch('vad_scores', max(total, 1) * model.n_states * 4)
    if total:
        ctx.gmm_loglik(d_feat, total, model.gmm_arrays(), d_sc)
    tokens = decode_device_scores(ctx, model, d_sc, off, timings)
    return tokens, last_frames


def decode_device_scores(ctx, model, d_scores, frame_off, timings=None):
    """Border shift (in place) and decoding of concatenated device scores [sum T, S]: the .exp
    token list [(first frame, word name)] of every file of frame_off."""
    if int(frame_off[-1]):
        ctx.vad_shift_batch(d_scores, frame_off, model.n_states, SHIFT_BORD)
        if timings is not None:
            timings.setdefault('vad_shift', []).append(ctx.last_ms('vad_shift'))
    stay, exit_, enter = model.decoder_constants()
    tok_off, frames, words, _ = ctx.vad_viterbi_batch(d_scores, frame_off, model.n_states, model.word_state,
                                                      stay, exit_, enter)
    if timings is not None and len(frame_off) > 1:
        timings.setdefault('vad_viterbi', []).append(ctx.last_ms('vad_viterbi'))
        timings.setdefault('vad_backtrack', []).append(ctx.last_ms('vad_backtrack'))
    return [[(int(t), model.words[w]) for t, w in zip(frames[a:b], words[a:b])]
            for a, b in zip(tok_off[:-1], tok_off[1:])]


def run(recipe, lnapath, exppath, model_path, device=0):
    """Every file of the recipe: .lna (shifted), .last_frame, .exp.  Returns the lna paths."""
    lnas = get_lnas(recipe, lnapath)
    model = VadModel.load(model_path)
    ctx = hipabi.Context(device)
    try:
        for wav, lna in lnas:
            pcm, rate = frontend.read_wav(wav)
            if rate != model.cfg.sample_rate:
                raise ValueError('%s is sampled at %d Hz, the model wants %d' % (wav, rate, model.cfg.sample_rate))
            write_scores_lna(lna, device_scores(ctx, model, pcm))
    finally:
        ctx.close()
    for _, lna in lnas:
        shift_dec_bord(lna, exppath)
    for _, lna in lnas:
        with open(op.join(exppath, op.splitext(op.basename(lna))[0] + '.exp'), 'w') as f:
            f.write(exp_text(model, lna_scores(lna)))
    return [lna for _, lna in lnas]


def run_self_trained(recipe, exppath, fcfg, opts=self_vad.SELF_VAD, device=0):
    """Every file of the recipe without a model (self_vad.decode_batch on the features of the
    configuration file fcfg, all files as one batch): .exp and .last_frame as run() leaves them, no
    .lna (there are no state scores of a model to keep).  A file the detector could not be trained on
    gets an empty .exp.  Returns the exp paths."""
    wavs = [wav for wav, _ in get_lnas(recipe, exppath)]
    cfg = feaconfig.FeatureConfig.load(fcfg)
    pcms = []
    for wav in wavs:
        pcm, rate = frontend.read_wav(wav)
        if rate != cfg.sample_rate:
            raise ValueError('%s is sampled at %d Hz, the feature configuration wants %d' % (wav, rate, cfg.sample_rate))
        pcms.append(pcm)
    ctx = hipabi.Context(device)
    try:
        d_pcm, sample_off = frontend.upload_batch(ctx, pcms)
        d_frames, frame_off = frontend.extract_batch(ctx, cfg, d_pcm, sample_off)
        tokens, last_frames = self_vad.decode_batch(ctx, opts, cfg, d_pcm, sample_off, d_frames, frame_off)
    finally:
        ctx.close()
    out = []
    for wav, toks, last in zip(wavs, tokens, last_frames):
        stem = op.join(exppath, op.splitext(op.basename(wav))[0])
        with open(stem + '.last_frame', 'w') as f:
            f.write('%d' % last)
        with open(stem + '.exp', 'w') as f:
            f.write(' '.join('%d %s' % (t, w) for t, w in toks))
        out.append(stem + '.exp')
    return out


def _create_argpath(argpath, say, ask):
    """generate_exp.py:78-91."""
    say('ERROR:', argpath, 'is not a valid directory.')
    create = ask('Attempt to create? [y/N]: ') or 'N'
    if create == 'y' or create == 'Y':
        try:
            os.mkdir(argpath)
        except Exception as e:
            say('Unable to create path:', e)
            return False
        return True
    say('Unable to continue without valid', argpath)
    return False


def main(argv=None, say=None, ask=input):
    """The reference's command line (generate_exp.py:19-31) through argparse, with its checks,
    refusals and progress lines (generate_exp.py:41-75).  -a / -t are accepted and not used:
    nothing here needs AaltoASR's phone_probs, Decoder module or test_token_pass.  Like the
    reference, a refusal prints its ERROR line and exits with status 0."""
    say = say or (lambda *a: print(*a, flush=True))
    ap = argparse.ArgumentParser(prog='generate_exp.py', description='Generate exp files: speech / non-speech '
                                 'scoring and decoding of the audio files of a recipe.')
    ap.add_argument('RECIPE', help='Recipe with audio files to process.')
    ap.add_argument('-l', '--lnapath', default='./lna', help='Choose a folder to drop the lna files [default: ./lna]; '
                    'accepted and unused with --self-trained, which writes no .lna')
    ap.add_argument('-e', '--exppath', default='./exp', help='Choose a folder to drop the exp files [default: ./exp]')
    ap.add_argument('-m', '--model', default='./hmms/mfcc_16g_11.10.2007_10',
                    help='Choose a model [default: ./hmms/mfcc_16g_11.10.2007_10]')
    ap.add_argument('-a', '--asrpath', default='./AaltoASR', help='Accepted and ignored (no AaltoASR needed)')
    ap.add_argument('-t', '--tokenpass', default='./VAD/tokenpass/test_token_pass',
                    help='Accepted and ignored (no test_token_pass needed)')
    ap.add_argument('--self-trained', dest='self_trained', metavar='FCONFIG', default=None,
                    help='No model: train the speech / non-speech detector on each recording itself, over the '
                         'features of this feature configuration file (fconfig.cfg); -m is not read, no .lna is written')
    ap.add_argument('--version', action='version', version='1.0')
    a = ap.parse_args(argv)
    if not op.exists(a.RECIPE):
        say('ERROR:', a.RECIPE, 'does not exist.')
        return 0
    if a.self_trained is not None:
        if not op.isdir(a.exppath) and not _create_argpath(a.exppath, say, ask):
            return 0
        if not op.isfile(a.self_trained):
            say('ERROR:', a.self_trained, 'does not exist.')
            return 0
        say('Reading recipe:', a.RECIPE)
        say('Self-trained detector on the features of:', a.self_trained)
        say('Writing `.exp` files in:', a.exppath)
        run_self_trained(a.RECIPE, a.exppath, a.self_trained)
        return 0
    for path in (a.lnapath, a.exppath):
        if not op.isdir(path) and not _create_argpath(path, say, ask):
            return 0
    if not op.isfile(a.model + '.cfg'):
        say('ERROR:', a.model, 'does not exist.')
        return 0
    say('Reading recipe:', a.RECIPE)
    say('Using model:', a.model)
    say('Writing `.lna` files in:', a.lnapath)
    say('Writing `.exp` files in:', a.exppath)
    run(a.RECIPE, a.lnapath, a.exppath, a.model)
    return 0
