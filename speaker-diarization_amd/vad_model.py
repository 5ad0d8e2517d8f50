"""Readers of the speech / non-speech model generate_exp.py decodes with (generate_exp.py:94-97,
189-239), in the AKU text formats of VAD/fileformats.html:

  MODEL.gk   Gaussian kernels: "K D diagonal_cov", then per kernel D means and D variances
  MODEL.mc   mixtures: "S", then per state "n k1 w1 .. kn wn" (kernels may be shared, weights 0)
  MODEL.ph   phones (Noway format): "PHONE", count, then per phone "index n_states label", the
             state line (-1 entry, -2 exit, mixture indices) and one transition line per state
  MODEL.cfg  the feature configuration (feaconfig.py)
  sp_nsp.lex lexicon lines "word(prob) phones"
  malli.bin  cis-binlm2 n-gram model (order 1 only)

and the one model object the decoder takes: a loop of words, each word one phone with exactly
one emitting state.  Any other topology, covariance type or n-gram order is refused (ValueError)
rather than reinterpreted.  Paths resolve like the reference: -m MODEL -> MODEL.{cfg,gk,mc,ph};
the lexicon and the language model are ./vad_models/sp_nsp.lex and ./vad_models/malli.bin
relative to the working directory (generate_exp.py:196-197).
"""
import math
import os
import re
import struct

import numpy as np

from .feaconfig import FeatureConfig

LEXICON = os.path.join('.', 'vad_models', 'sp_nsp.lex')
NGRAM = os.path.join('.', 'vad_models', 'malli.bin')

# decoder settings of generate_exp.py:221-224
TRANSITION_SCALE, LM_SCALE, INSERTION_PENALTY = 2.0, 10.0, 1.0


def read_gk(path):
    """(means [K, D], variances [K, D]) in float64; diagonal covariances only."""
    with open(path) as f:
        head = f.readline().split()
        if len(head) < 3:
            raise ValueError('%s: expected "kernels dim type" on the first line' % path)
        k, d, kind = int(head[0]), int(head[1]), head[2]
        if kind != 'diagonal_cov':
            raise ValueError('%s: %s kernels are not supported (this build reads diagonal_cov)' % (path, kind))
        rows = [line.split() for line in f if line.strip()]
    if len(rows) != k or any(len(r) != 2 * d for r in rows):
        raise ValueError('%s: expected %d kernels of %d means and %d variances' % (path, k, d, d))
    a = np.array(rows, dtype=np.float64).reshape(k, 2 * d)
    means, variances = a[:, :d].copy(), a[:, d:].copy()
    if not np.all(np.isfinite(means)) or not np.all(np.isfinite(variances)) or not np.all(variances > 0):
        raise ValueError('%s: means must be finite and variances finite and positive' % path)
    return means, variances


def read_mc(path):
    """[(kernel indices int array, weights float64 array)] per state."""
    with open(path) as f:
        toks = f.read().split()
    if not toks:
        raise ValueError('%s: empty mixture file' % path)
    n, i, states = int(toks[0]), 1, []
    for _ in range(n):
        m = int(toks[i])
        pairs = toks[i + 1:i + 1 + 2 * m]
        if len(pairs) != 2 * m:
            raise ValueError('%s: truncated state line' % path)
        states.append((np.array([int(x) for x in pairs[0::2]], dtype=np.int64),
                       np.array([float(x) for x in pairs[1::2]], dtype=np.float64)))
        i += 1 + 2 * m
    if i != len(toks):
        raise ValueError('%s: %d states declared, more numbers follow' % (path, n))
    return states


def read_ph(path):
    """[{'index', 'label', 'states': [..], 'trans': {relative state: [(to, prob), ..]}}]."""
    with open(path) as f:
        lines = [line.split() for line in f if line.strip()]
    if not lines or lines[0] != ['PHONE']:
        raise ValueError('%s: a phone file begins with PHONE' % path)
    n, i, phones = int(lines[1][0]), 2, []
    for _ in range(n):
        index, n_states, label = int(lines[i][0]), int(lines[i][1]), lines[i][2]
        states = [int(x) for x in lines[i + 1]]
        if len(states) != n_states:
            raise ValueError('%s: phone %s declares %d states, lists %d' % (path, label, n_states, len(states)))
        trans = {}
        for line in lines[i + 2:i + 2 + n_states]:
            rel, cnt = int(line[0]), int(line[1])
            if len(line) != 2 + 2 * cnt or rel in trans:
                raise ValueError('%s: bad transition line %r of phone %s' % (path, ' '.join(line), label))
            trans[rel] = [(int(line[2 + 2 * k]), float(line[3 + 2 * k])) for k in range(cnt)]
        if sorted(trans) != list(range(n_states)):
            raise ValueError('%s: phone %s needs one transition line per state' % (path, label))
        phones.append({'index': index, 'label': label, 'states': states, 'trans': trans})
        i += 2 + n_states
    if i != len(lines):
        raise ValueError('%s: %d phones declared, more lines follow' % (path, n))
    return phones


_LEX = re.compile(r'^(\S+?)(?:\(([^)]*)\))?\s+(.+)$')


def read_lex(path):
    """[(word, probability, [phones])] in file order."""
    out = []
    with open(path) as f:
        for line in f:
            if not line.strip():
                continue
            m = _LEX.match(line.strip())
            if not m:
                raise ValueError('%s: bad lexicon line %r' % (path, line))
            out.append((m.group(1), float(m.group(2)) if m.group(2) else 1.0, m.group(3).split()))
    return out


def read_binlm(path):
    """cis-binlm2 unigram model: (vocabulary, {word: log10 probability}).  Header lines
    "cis-binlm2", the model type, the vocabulary size and words, "order nodes", the count of
    each order; then per node 16 little-endian bytes (int32 word, float32 log10 p, float32
    back-off, int32 child)."""
    with open(path, 'rb') as f:
        data = f.read()
    pos = [0]

    def line():
        j = data.index(b'\n', pos[0])
        s = data[pos[0]:j].decode('latin-1')
        pos[0] = j + 1
        return s

    if line() != 'cis-binlm2':
        raise ValueError('%s: not a cis-binlm2 file' % path)
    kind = line()
    if kind not in ('backoff', 'interpolated'):
        raise ValueError('%s: unknown model type %r' % (path, kind))
    vocab = [line() for _ in range(int(line()))]
    order, n_nodes = [int(x) for x in line().split()]
    if order != 1:
        raise ValueError('%s: n-gram order %d is not supported (the decoder here takes unigrams)' % (path, order))
    counts = [int(line()) for _ in range(order)]
    if counts[0] != n_nodes or len(data) - pos[0] != 16 * n_nodes:
        raise ValueError('%s: %d unigram nodes declared, %d bytes follow' % (path, n_nodes, len(data) - pos[0]))
    logp = {}
    for k in range(n_nodes):
        word, lp, _bo, _child = struct.unpack_from('<iffi', data, pos[0] + 16 * k)
        if not 0 <= word < len(vocab):
            raise ValueError('%s: node %d names word %d of %d' % (path, k, word, len(vocab)))
        logp[vocab[word]] = float(lp)
    return vocab, logp


class VadModel(object):
    """The word loop the decoder runs and the Gaussian mixtures that score its states."""

    def __init__(self, gk, mc, ph, lex, lm, cfg=None):
        self.means, self.variances = gk
        self.n_kernels, self.dim = self.means.shape
        self.mixtures = mc
        self.n_states = len(mc)
        for s, (ks, ws) in enumerate(mc):
            if len(ks) and (ks.min() < 0 or ks.max() >= self.n_kernels):
                raise ValueError('mixture %d names a kernel outside 0..%d' % (s, self.n_kernels - 1))
            if not np.all(np.isfinite(ws)) or np.any(ws < 0):
                raise ValueError('mixture %d has a negative or non-finite weight' % s)
        by_label = {}
        for p in ph:
            by_label[p['label']] = self._one_state_phone(p)
        vocab, logp = lm
        self.words, self.word_state, self.a_stay, self.a_exit, self.log10p = [], [], [], [], []
        for word, _prob, phones in lex:
            if len(phones) != 1:
                raise ValueError('word %s has %d phones; the decoder here takes one-phone words' % (word, len(phones)))
            if phones[0] not in by_label:
                raise ValueError('word %s uses phone %s, which the phone file lacks' % (word, phones[0]))
            if word not in logp:
                raise ValueError('word %s is not in the language model' % word)
            state, stay, exit_ = by_label[phones[0]]
            self.words.append(word)
            self.word_state.append(state)
            self.a_stay.append(stay)
            self.a_exit.append(exit_)
            self.log10p.append(logp[word])
        if not self.words:
            raise ValueError('empty lexicon')
        self.cfg = cfg

    def _one_state_phone(self, p):
        """(mixture index, a_stay, a_exit) of a phone -1 -> s -> -2 with a self loop; anything else raises."""
        st, tr = p['states'], p['trans']
        if len(st) != 3 or st[0] != -1 or st[1] != -2 or st[2] < 0:
            raise ValueError('phone %s: only phones of one emitting state are supported (got states %r)' % (p['label'], st))
        if st[2] >= self.n_states:
            raise ValueError('phone %s: state %d has no mixture' % (p['label'], st[2]))
        out = dict(tr[2])
        if [t for t, _ in tr[0]] != [2] or tr[1] or sorted(out) != [1, 2] or len(tr[2]) != 2:
            raise ValueError('phone %s: transitions %r are not entry -> state, self loop, state -> exit' % (p['label'], tr))
        return st[2], out[2], out[1]

    @classmethod
    def load(cls, model, lexicon=LEXICON, ngram=NGRAM):
        """-m MODEL: MODEL.{cfg,gk,mc,ph}; lexicon and LM where the reference looks for them."""
        return cls(read_gk(model + '.gk'), read_mc(model + '.mc'), read_ph(model + '.ph'), read_lex(lexicon),
                   read_binlm(ngram), FeatureConfig.load(model + '.cfg'))

    def gmm_arrays(self):
        """The arrays spkd_gmm_loglik takes: 1/v, ln w and c_k = -1/2 (D ln 2pi + sum ln v) formed
        in float64, handed over as float32."""
        with np.errstate(divide='ignore'):
            lw = [np.log(ws) for _, ws in self.mixtures]
        off = np.zeros(self.n_states + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(ks) for ks, _ in self.mixtures])
        c = -0.5 * (self.dim * math.log(2.0 * math.pi) + np.log(self.variances).sum(axis=1))
        return {'mean': self.means.astype(np.float32), 'inv_var': (1.0 / self.variances).astype(np.float32),
                'log_norm': c.astype(np.float32), 'state_off': off,
                'kernel': np.concatenate([ks for ks, _ in self.mixtures] + [np.zeros(0, np.int64)]).astype(np.int32),
                'log_weight': np.concatenate(lw + [np.zeros(0)]).astype(np.float32)}

    def decoder_constants(self, ts=TRANSITION_SCALE, lm=LM_SCALE, ins=INSERTION_PENALTY):
        """(stay, exit, enter) per word, float64: ts ln a_jj, ts ln a_j,exit, lm ln(10) log10 P(j) - ins."""
        with np.errstate(divide='ignore'):
            stay = ts * np.log(np.array(self.a_stay, dtype=np.float64))
            exit_ = ts * np.log(np.array(self.a_exit, dtype=np.float64))
        enter = lm * np.log(10.0) * np.array(self.log10p, dtype=np.float64) - ins
        return stay, exit_, enter
