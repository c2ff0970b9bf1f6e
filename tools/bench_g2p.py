"""Latency of the word-level G2P decoder (networks.g2p.G2P: words in, transcriptions out, host work and the read-back of the labels included) for one
sentence of about 20 words and for 64 ragged sentences, two formulations of the same loop on the same weights in the same process:
  hip     g2p_embed -> LSTMHip -> two hoisted linear_hip -> ttsc_g2p_decode: one launch for all words of the call, per-word stop
  torch   the reference's loop restated in torch ops on the GPU (nn.Embedding, nn.LSTM encoder, per step: cat / matmul / tanh / bmm / softmax /
          bmm, one nn.LSTM step, nn.Linear, argmax, embedding; batch-wide stop with one host read per step, as modules.py:271-295).  A batch
          shares one N there, so the ragged case runs sentence by sentence — the only way that formulation gives every word its own sentence's
          padding, i.e. the same loop on the same inputs; `torch_global_n` pads all 64 sentences to one N instead: one batch and far fewer
          launches, but another computation (the reference attends over the padding), whose transcriptions differ — it is timed and its
          differing words are counted so that the log shows both, and it is not part of the gate.
Weights: the seeded fixture weights of tests/golden/g2p_c.npz (words stop after 6-8 steps, a few run to 10 N + 1).  No lexicon: every word is decoded.
Before timing, each case compares the labels of hip and torch word by word.  Two fp32 implementations of a free-running loop part for good at the
first step where the top two logits lie closer than their rounding differences, so for every differing word the log records the step of the
first differing label and the top-2 logit margin there, on both sides (up to that step both loops were fed the same labels, so their logits
agree to rounding).  A margin below 2e-4 (twice the project's 1e-4 logit gate, the fixtures' rule) is a near-tie; anything larger would be a
difference in what is computed.  The recorded run (profiles/g2p_bench.log): 0 of 21 and 18 of 953 words differ, every one at a margin <= 2.4e-7;
with one global N, 291 of 953 transcriptions differ.
Wall-clock medians after a warm-up, the formulations timed alternately.  Exit status 1 unless hip is faster than torch by more than the 1.5 %
box-to-box spread at both sizes and every differing word parts at a near-tie.
    python tools/bench_g2p.py [--reps 5] [--rounds 5]      (the JSON line is also written to profiles/g2p_bench.log)"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

SENTENCE = "good morning and welcome to the world of speech synthesis don't feel bad about us we're only here to help you".split()
WORDS = "the quick brown fox jumps over a lazy dog while it's raining cats and dogs in spain doesn't it yes no maybe never extraordinarily".split()
SPREAD = 0.015
NEAR_TIE = 2e-4


def ragged_sentences(n, seed=7):
    rng = np.random.RandomState(seed)
    return [list(rng.choice(WORDS, size=rng.randint(3, 30))) for _ in range(n)]


def torch_transcribe(g2p, words, N, raw=False):
    """the reference's Seq2Seq.forward(x) + G2P.transcribe in torch ops on the device; raw: -> (labels [B, T], logits [B, T, L]) instead"""
    net = g2p.seq2seq
    dev = net.input_emb.weight.device
    with torch.no_grad():
        x = torch.from_numpy(g2p.encode_words(words, N)).to(dev)
        enc, _ = net.encoder(net.input_emb(x))
        B = x.shape[0]
        _, hidden = net.decoder(torch.zeros((B, 1, net._dec_input_size), device=dev))
        last = torch.zeros((B, net.emb_size), device=dev)
        w_att, b_att, v = net.attention.attn.conv.weight[:, :, 0], net.attention.attn.conv.bias, net.attention.v
        done = torch.zeros(B, dtype=torch.bool, device=dev)
        labels, logits = [], []
        for index in range(10 * N + 1):
            q = hidden[-1][-1].unsqueeze(1).expand(-1, N, -1)
            energy = torch.tanh(torch.cat((q, enc), dim=2) @ w_att.t() + b_att)
            att = torch.softmax(torch.bmm(energy, v.expand(B, -1).unsqueeze(2)).squeeze(2), dim=1)
            ctx = torch.bmm(att.unsqueeze(1), enc).squeeze(1)
            out, hidden = net.decoder(torch.cat([ctx, last], dim=1).unsqueeze(1), hx=hidden)
            lg = net.output(out.squeeze(1))
            outp = torch.argmax(lg, dim=1)
            labels.append(outp)
            if raw:
                logits.append(lg)
            last = net.output_emb(outp)
            done |= outp == net._EOS
            if bool(done.all()):
                break
        lab = torch.stack(labels, dim=1).cpu().numpy()
        if raw:
            return lab, torch.stack(logits, dim=1).cpu().numpy()
    return [g2p.labels_to_phones(row.tolist()) for row in lab]


def used(g2p, row, cap):
    """the labels transcribe reads: up to and including the first <EOS>, at most cap"""
    row = [int(v) for v in row[:cap]]
    eos = g2p.label2int['<EOS>']
    return row[:row.index(eos) + 1] if eos in row else row


def top2_margin(lg):
    top = np.sort(np.asarray(lg, dtype=np.float64))[-2:]
    return float(top[1] - top[0])


def compare(g2p, words, ns, torch_raw):
    """hip against torch, word by word.  torch_raw: per word (labels row, logits rows) of the torch loop.
    -> (words differing in their transcription, words differing in their used labels, [(word, n, step, hip margin, torch margin)])"""
    net = g2p.seq2seq
    N = max(ns)
    x = torch.from_numpy(g2p.encode_words(words, N)).to(net.input_emb.weight.device)
    n = None if all(v == N for v in ns) else list(ns)
    idx, count = net.transcribe_ids(x, n=n)
    idx, count = idx.cpu().numpy(), count.cpu().numpy()
    first = {}
    tr_diff = 0
    for i, (lab_t, _) in enumerate(torch_raw):
        h, t = used(g2p, idx[i, :count[i]], 10 * ns[i] + 1), used(g2p, lab_t, 10 * ns[i] + 1)
        tr_diff += int(g2p.labels_to_phones(h) != g2p.labels_to_phones(t))
        if h != t:
            first[i] = next((s for s, (p, q) in enumerate(zip(h, t)) if p != q), min(len(h), len(t)))
    parts = []
    if first:
        sel = sorted(first)
        T = max(first.values()) + 1
        with torch.no_grad():         # the fixed-steps mode on the differing words alone (a word's bits do not depend on the launch)
            xs = x[sel]
            nsel = None if n is None else [ns[i] for i in sel]
            lg = net.decode(net.encode(xs, nsel), n=nsel, steps=T, want_idx=False)[2].cpu().numpy()
        for k, i in enumerate(sel):
            s = first[i]
            parts.append((words[i], ns[i], s, top2_margin(lg[k, s]), top2_margin(torch_raw[i][1][s])))
    return tr_diff, len(first), parts


def wall_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    a = ap.parse_args()
    from oracle import meldecoder_ref as M
    from ttscube_amd.networks.g2p import G2P
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'g2p_c.npz'))
    obj = json.loads(str(g['enc']))
    g2p = G2P()
    g2p.token2int, g2p.label2int, g2p.label_list = obj['token2int'], obj['label2int'], obj['label_list']
    g2p.initialize_network()
    sd = M.fill_state_dict([(k, tuple(s)) for k, s in json.loads(str(g['shapes']))], int(g['seed']))
    sd['output.bias'][2] += float(g['eos_offset'])
    g2p.seq2seq.load_state_dict(sd, strict=True)
    g2p.eval()
    g2p.to('cuda:0')
    g2p.seq2seq.encoder.flatten_parameters()
    g2p.seq2seq.decoder.flatten_parameters()
    sents = ragged_sentences(64)
    ns = [max(len(w) for w in s) + 1 for s in sents]
    flat_words = [w for s in sents for w in s]
    flat_ns = [n for s, n in zip(sents, ns) for _ in s]
    n1 = max(len(w) for w in SENTENCE) + 1
    cases = {
        'one_sentence_%d_words' % len(SENTENCE): {
            'hip': lambda: g2p._decode_words(SENTENCE, [n1] * len(SENTENCE)),
            'torch': lambda: torch_transcribe(g2p, SENTENCE, n1)},
        'batch_64_ragged_%d_words' % len(flat_words): {
            'hip': lambda: g2p._decode_words(flat_words, flat_ns),
            'torch': lambda: [torch_transcribe(g2p, s, n) for s, n in zip(sents, ns)],
            'torch_global_n': lambda: torch_transcribe(g2p, flat_words, max(ns))},
    }
    def torch_rows(words_of, ns_of):
        rows = []
        for ws, n in zip(words_of, ns_of):
            lab, lg = torch_transcribe(g2p, ws, n, raw=True)
            rows += [(lab[i], lg[i]) for i in range(len(ws))]
        return rows

    checks = {
        'one_sentence_%d_words' % len(SENTENCE): (SENTENCE, [n1] * len(SENTENCE), lambda: torch_rows([SENTENCE], [n1])),
        'batch_64_ragged_%d_words' % len(flat_words): (flat_words, flat_ns, lambda: torch_rows(sents, ns)),
    }
    out = {'reps': a.reps, 'rounds': a.rounds, 'near_tie_margin': NEAR_TIE}
    ok = ties = True
    for cname, forms in cases.items():
        words, wns, rows = checks[cname]
        tr_diff, lab_diff, parts = compare(g2p, words, wns, rows())
        for f in forms.values():
            for _ in range(a.warmup):
                f()
        res = {k: [] for k in forms}
        for _ in range(a.rounds):
            for k, f in forms.items():
                res[k].append(wall_ms(f, a.reps))
        r = {k + '_ms_median': float(np.median(v)) for k, v in res.items()}
        r['torch_over_hip'] = r['torch_ms_median'] / r['hip_ms_median']
        r['words'] = len(words)
        r['words_whose_transcription_differs_from_torch'] = tr_diff
        r['words_whose_labels_differ_from_torch'] = lab_diff
        margins = [max(m_hip, m_torch) for _, _, _, m_hip, m_torch in parts]
        r['largest_top2_margin_at_a_first_differing_step'] = max(margins) if margins else None
        r['differing_words_part_at_a_near_tie'] = all(m < NEAR_TIE for m in margins)
        r['first_differing_steps'] = [{'word': w, 'n': n, 'step': s, 'hip_margin': mh, 'torch_margin': mt} for w, n, s, mh, mt in parts[:20]]
        if 'torch_global_n' in forms:
            rows_g = torch_transcribe(g2p, words, max(wns), raw=True)
            r['torch_global_n_words_whose_transcription_differs'] = compare(g2p, words, wns, list(zip(*rows_g)))[0]
        ties = ties and r['differing_words_part_at_a_near_tie']
        ok = ok and r['hip_ms_median'] * (1 + SPREAD) < r['torch_ms_median']
        out[cname] = r
    out['gate_hip_faster_than_torch_at_both_sizes'] = ok
    out['gate_differing_words_part_at_near_ties'] = ties
    ok = ok and ties
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'g2p_bench.log'), 'w') as f:
        f.write('python tools/bench_g2p.py --reps %d --rounds %d\n%s\n' % (a.reps, a.rounds, line))
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
