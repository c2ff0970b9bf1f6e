"""CPU: the G2P training surface without a device — no CPU path, the trainer's flag table, the batch construction and the fixture's own check."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from tests.conftest import ROOT

GOLD = os.path.join(ROOT, 'tests', 'golden')


def _g2p():
    from ttscube_amd.networks.g2p import G2P
    g2p = G2P()
    with open(os.path.join(GOLD, 'g2p.encodings')) as f:
        enc = json.load(f)
    g2p.token2int, g2p.label2int, g2p.label_list = enc['token2int'], enc['label2int'], enc['label_list']
    return g2p


def test_host_tensors_raise():
    from ttscube_amd import _lib
    from ttscube_amd.networks import g2p_train as GT
    from ttscube_amd.networks.lstm_autograd import lstm_forward_train
    g2p = _g2p()
    g2p.initialize_network()
    with pytest.raises(_lib.TTSCError, match='no CPU path'):
        GT.learn_batch(g2p, [('ab', ['AH0', 'B'])])
    net = g2p.seq2seq
    with pytest.raises(_lib.TTSCError, match='no CPU path'):
        GT.decoder_forward_train(net, torch.zeros(1, 3, 400), torch.ones(1, 2, dtype=torch.long))
    with pytest.raises(_lib.TTSCError, match='no CPU path'):
        lstm_forward_train(net.encoder, torch.zeros(1, 3, 100), dropout_seed=1)


def test_make_batch_builds_the_reference_arrays():
    from ttscube_amd.networks import g2p_train as GT
    z = np.load(os.path.join(GOLD, 'g2p_train_a.npz'))
    g2p = _g2p()
    x, y = GT.make_batch(g2p, [(w, t) for w, t in json.loads(str(z['batches']))[0]])
    assert x.dtype == np.int64 and np.array_equal(x, z['x']) and np.array_equal(y, z['y'])
    x, y = GT.make_batch(g2p, [('a?', ['AH0']), ('b', ['B', 'no-such-phone', 'IY1'])])
    assert x.shape == (2, 3) and y.shape == (2, 4)
    assert x[0, 1] == 1 and x[0, 2] == 2 and x[1, 1] == 2 and x[1, 2] == 0          # <UNK>, <EOS>, then <PAD>
    assert y[1, 1] == 1 and y[1, 3] == 2 and y[0, 1] == 2 and y[0, 2] == 0


def test_trainer_flags_are_the_reference_options():
    spec = importlib.util.spec_from_file_location('train_g2p', os.path.join(ROOT, 'scripts', 'train_g2p.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    want = {'--train-file': 'train_file', '--dev-file': 'dev_file', '--store': 'output_path', '--batch-size': 'batch_size', '--lr': 'lr',
            '--patience': 'patience', '--load': 'model_path', '--device': 'device', '--resume': 'resume'}
    assert {f[0]: f[1] for f in mod.REFERENCE_FLAGS} == want
    ns = mod.parser().parse_args(['--train-file', 'a', '--dev-file', 'b', '--store', 'c'])
    assert (ns.batch_size, ns.lr, ns.patience, ns.device, ns.model_path, ns.resume) == (32, 1e-3, 20, 'cuda:0', None, False)
    assert mod.get_batches(list(range(5)), 2) == [[0, 1], [2, 3], [4]] and mod.get_batches(list(range(4)), 2) == [[0, 1], [2, 3]]


def test_fixture_replay_check_is_within_the_gates():
    z = np.load(os.path.join(GOLD, 'g2p_train_b.npz'))
    assert 0.0 <= float(z['replay_check']) <= 1e-4
    # the float64 helper reproduces the stored loss from the stored masks (what the generator checked, again, on this machine)
    from oracle import meldecoder_ref as M
    from tests import g2p_train_reference as R
    shapes = [(k, tuple(s)) for k, s in json.loads(str(z['shapes']))]
    P = R.leaves(M.fill_state_dict(shapes, int(z['seed'])))
    un = lambda k, n: torch.from_numpy(np.unpackbits(z[k], axis=-1)[..., :n].astype(np.float32))
    masks = {'att': list(un('mask_att', 200))}
    if int(z['lstm_dropout']):
        masks.update(enc=un('mask_enc', 400), init=un('mask_init', 200), dec=list(un('mask_dec', 200)))
    p = 0.33 if int(z['lstm_dropout']) else 0.0
    with torch.no_grad():
        lg = R.seq2seq_reference(P, torch.from_numpy(z['x']), torch.from_numpy(z['y']), masks, p_enc=p, p_dec=p)
        loss = R.loss_reference(lg, torch.from_numpy(z['y']))
    assert abs(float(loss) - float(z['loss'])) <= 1e-4
    assert float((lg - torch.from_numpy(z['logits']).double()).abs().max()) <= 1e-4
