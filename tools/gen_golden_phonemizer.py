"""Golden vectors for the sentence phonemizer, produced by the REFERENCE ITSELF (build container only; the reference never travels).

    python tools/gen_golden_phonemizer.py   ->  tests/golden/phonemizer_{a,b,long}.npz, phonemizer_train_{a,b}.npz, phonemizer_collate.npz,
                                                phonemizer_dev.json, phonemizer.encodings

phonemizer_dev.json / phonemizer.encodings: a subset of the reference's data/blizzard-g2p.dev and its data/phonemizer-blizzard.encodings (data its
programs read).  Inference fixtures: the reference's CubenetPhonemizer with seeded weights (oracle.meldecoder_ref.fill_state_dict: the fixture
stores seed + shapes), its logits and arg-max tags on one text, and the dict the reference's Text2FeatBlizzard returns for that text.  The
generator prints every fixture's smallest top-2 logit margin; `phonemizer_a` (the fixture the front-end test compares whole dicts on) is refused
below 2e-4, the others when more than 5 % of their positions lie below it.  Train fixtures: a padded batch of dev-subset examples (one target
per character), the reference's training_step loss, its logits and the gradient of every parameter — whole for tensors of up to SAMPLE
elements, SAMPLE evenly strided elements plus the norm / probe fingerprint (oracle/fingerprint.py) for larger ones."""
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import ref_import  # noqa: E402

ref_import.setup()
from cube.io_utils.io_phonemizer import PhonemizerCollate, PhonemizerEncodings  # noqa: E402
from cube.io_utils.io_text import Text2FeatBlizzard  # noqa: E402
from cube.networks.phonemizer import CubenetPhonemizer  # noqa: E402
from oracle import meldecoder_ref as M  # noqa: E402
from oracle.fingerprint import fingerprint  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
REF_DATA = os.path.join(ref_import.REF, 'data')
SAMPLE = 1024
MARGIN = 2e-4
N_DEV = 16

TEXTS = {
    'a': "Don't go,\nBob!\n\nYes: it's ok.",
    'b': "Good morning, and welcome to the world of speech synthesis!\nDon't feel bad about us; we're only here to help.\n\nAre you ready?",
    'long': ("It was the best of times, it was the worst of times; it was the age of wisdom, it was the age of foolishness.\n"
             "Nobody's fault, said Mr. Pickwick, smiling: \"Isn't it a fine morning?\"\n\n"
             "The quick brown fox jumps over the lazy dog, twice, and then once more for good measure. Weren't they tired? No!\n"
             "Charles's letters arrived on Tuesday, Wednesday and Friday.\n\nThat's all, folks: the end of the second paragraph is here."),
}


def dev_subset():
    with open(os.path.join(REF_DATA, 'blizzard-g2p.dev')) as f:
        exs = json.load(f)
    exs = [e for e in exs if len(e['phones']) == len(e['orig_text']) and 'hybrid' in e and len(e['orig_text']) <= 64]
    return exs[:N_DEV]


def seeded(enc, seed):
    torch.manual_seed(0)
    net = CubenetPhonemizer(enc)
    shapes = M.named_shapes(net)
    net.load_state_dict(M.fill_state_dict(shapes, seed), strict=True)
    return net, shapes


def margins(logits):
    top = torch.topk(logits, 2, dim=-1).values
    return (top[..., 0] - top[..., 1]).reshape(-1).numpy()


def gen_infer(name, seed, enc, enc_json):
    text = TEXTS[name]
    net, shapes = seeded(enc, seed)
    net.eval()
    with tempfile.TemporaryDirectory() as tmp:
        base = os.path.join(tmp, 'phonemizer')
        enc.save(base + '.encodings')
        net.save(base + '.model')
        t2f = Text2FeatBlizzard(base)
        rez = t2f(text)
        with torch.no_grad():
            X = t2f._collate.collate_fn([{'orig_text': rez['orig_text'], 'phones': ['1'], 'phon2word': [1], 'words': ['1']}])
            logits = t2f._phonemizer(X)
    mg = margins(logits)
    low = float((mg < MARGIN).mean())
    print('%s seed %d: %d characters, logit rms %.3f, min margin %.3e, share below %.0e: %.2f %%'
          % (name, seed, X['x_char'].shape[1], float(logits.pow(2).mean().sqrt()), mg.min(), MARGIN, 100 * low))
    if name == 'a' and mg.min() < MARGIN:
        raise SystemExit('phonemizer_a: minimum margin below %g — pick another seed / text' % MARGIN)
    if low > 0.05:
        raise SystemExit('phonemizer_%s: more than 5 %% of the positions lie below the margin — pick another seed / text' % name)
    np.savez_compressed(os.path.join(OUT, 'phonemizer_%s.npz' % name), seed=seed, shapes=json.dumps(shapes), enc=enc_json, text=text,
                        x_char=X['x_char'].numpy(), x_case=X['x_case'].numpy(), logits=logits.numpy(),
                        tags=torch.argmax(logits, dim=-1).numpy(), result=json.dumps(rez))


def gen_train(name, seed, enc, enc_json, exs):
    net, shapes = seeded(enc, seed)
    net.train()
    # one target per character: without `hybrid` the reference's collate takes `phones`; its phon2word must then be per character as well
    exs = [dict({k: v for k, v in e.items() if k != 'hybrid'}, phon2word=[i for i, w in enumerate(e['words']) for _ in w]) for e in exs]
    batch = PhonemizerCollate(enc).collate_fn(exs)
    assert batch['y_phon'].shape == batch['x_char'].shape and int((batch['y_phon'] == 0).sum()) > 0
    loss = net.training_step(batch, 0)
    loss.backward()
    with torch.no_grad():
        logits = net.forward(batch)
    out = dict(seed=seed, shapes=json.dumps(shapes), enc=enc_json, x_char=batch['x_char'].numpy(), x_case=batch['x_case'].numpy(),
               y_phon=batch['y_phon'].numpy(), lengths=np.asarray([len(e['orig_text']) for e in exs]), loss=np.float64(loss.item()),
               logits=logits.numpy(), grad_names=json.dumps([k for k, _ in net.named_parameters()]))
    for k, p in net.named_parameters():
        g = p.grad.detach().numpy().reshape(-1)
        if g.size <= SAMPLE:
            out['grad/%s/full' % k] = g
            continue
        fp = fingerprint(g, k)
        idx = np.unique(np.linspace(0, g.size - 1, SAMPLE).astype(np.int64))
        out.update({'grad/%s/idx' % k: idx, 'grad/%s/samples' % k: g[idx], 'grad/%s/norm' % k: fp['norm'], 'grad/%s/probe' % k: fp['probe'],
                    'grad/%s/size' % k: fp['size']})
    np.savez_compressed(os.path.join(OUT, name + '.npz'), **out)
    print(name, 'batch', tuple(batch['x_char'].shape), 'loss', loss.item())


def gen_data():
    exs = dev_subset()
    with open(os.path.join(OUT, 'phonemizer_dev.json'), 'w') as f:
        json.dump(exs, f)
    with open(os.path.join(REF_DATA, 'phonemizer-blizzard.encodings')) as f:
        enc_json = f.read()
    with open(os.path.join(OUT, 'phonemizer.encodings'), 'w') as f:
        f.write(enc_json)
    enc = PhonemizerEncodings(os.path.join(OUT, 'phonemizer.encodings'))
    b = PhonemizerCollate(enc).collate_fn(exs)
    np.savez_compressed(os.path.join(OUT, 'phonemizer_collate.npz'), x_words=json.dumps(b['x_words']),
                        **{k: v.numpy() for k, v in b.items() if torch.is_tensor(v)})
    print('phonemizer_dev.json: %d examples, %d graphemes, %d phones' % (len(exs), len(enc.graphemes), len(enc.phonemes)))
    return exs, enc, enc_json


if __name__ == '__main__':
    exs, enc, enc_json = gen_data()
    for name, seed in (('a', 11), ('b', 12), ('long', 13)):
        gen_infer(name, seed, enc, enc_json)
    gen_train('phonemizer_train_a', 21, enc, enc_json, exs[:4])
    gen_train('phonemizer_train_b', 22, enc, enc_json, exs)
