"""GPU: CubenetTextcoder training (networks/textcoder_train.py, csrc/textcoder_train.hip).

  * the BatchNorm -> tanh -> dropout kernels against float64 torch (outputs / running statistics <= 1e-5, gradients <= 1e-4 relative, bit-identical
    repeats), and the Philox mask path — the per-element statement of these kernels and of the loss (every dispatch path, |got - ref64| <=
    tau * S with no absolute floor) is tests/test_text_train_f64_gpu.py;
  * the loss kernel against float64 torch (ignored rows, ignore_index >= classes, an all-ignored head) and its out-of-range status;
  * reference parity (tests/golden/textcoder_train_{a,b,pf1}.npz, made by the reference itself): outputs, losses, every gradient and the running
    statistics after a step, every parameter after two Adam steps — the gate of the Languasito2 training parity test (1e-4 relative);
  * determinism of a 3-step run, eval mode after training, and the trainer script end to end with --resume."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import meldecoder_ref as M
from oracle.fingerprint import compare
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _bn_ref(x, g, b, rm, rv, mask, p=0.1, momentum=0.1, eps=1e-5):
    x, g, b = x.double().requires_grad_(True), g.double().requires_grad_(True), b.double().requires_grad_(True)
    rm, rv = rm.double().clone(), rv.double().clone()
    y = torch.tanh(F.batch_norm(x, rm, rv, g, b, training=True, momentum=momentum, eps=eps)) * mask.double() / (1 - p)
    return y, x, g, b, rm, rv


@pytest.mark.parametrize('B', [1, 3, 16])
@pytest.mark.parametrize('Fr', [1, 7, 601])
def test_bn_tanh_dropout_kernels_match_float64_torch(B, Fr):
    from ttscube_amd import _lib
    from ttscube_amd.networks.textcoder_train import BnTanhDropoutFn
    gen = torch.Generator().manual_seed(B * 1000 + Fr)
    C_ = 512
    x = (torch.randn(B, C_, Fr, generator=gen) * 1.5 + 0.3).cuda()
    g = (torch.rand(C_, generator=gen) + 0.5).cuda()
    b = (torch.randn(C_, generator=gen) * 0.2).cuda()
    rm0 = (torch.randn(C_, generator=gen) * 0.1).cuda()
    rv0 = (torch.rand(C_, generator=gen) + 0.5).cuda()
    mask = (torch.rand(B, C_, Fr, generator=gen) > 0.1).float().cuda()
    dy = torch.randn(B, C_, Fr, generator=gen).cuda()
    if B * Fr == 1:      # torch's BatchNorm raises here ("Expected more than 1 value per channel"); so does the kernel's host side
        with pytest.raises(_lib.TTSCError):
            BnTanhDropoutFn.apply(x, g, b, rm0.clone(), rv0.clone(), mask, 0, 0, 0.1, 1e-5, 0.1)
        return
    runs = []
    for _ in range(2):
        rm, rv = rm0.clone(), rv0.clone()
        xg, gg, bg = x.clone().requires_grad_(True), g.clone().requires_grad_(True), b.clone().requires_grad_(True)
        y = BnTanhDropoutFn.apply(xg, gg, bg, rm, rv, mask, 0, 0, 0.1, 1e-5, 0.1)
        y.backward(dy)
        runs.append([t.detach().cpu() for t in (y, rm, rv, xg.grad, gg.grad, bg.grad)])
    for a, c in zip(runs[0], runs[1]):
        assert torch.equal(a, c)                      # fixed-order reductions: the same bits twice
    yr, xr, gr, br, rmr, rvr = _bn_ref(x.cpu(), g.cpu(), b.cpu(), rm0.cpu(), rv0.cpu(), mask.cpu())
    yr.backward(dy.cpu().double())
    y, rm, rv, dx, dg, db = runs[0]
    assert _rel(y, yr.detach()) <= 1e-5
    assert _rel(rm, rmr) <= 1e-5 and _rel(rv, rvr) <= 1e-5
    assert _rel(dx, xr.grad) <= 1e-4 and _rel(dg, gr.grad) <= 1e-4 and _rel(db, br.grad) <= 1e-4


def test_bn_tanh_dropout_philox_mask_is_consistent_between_passes():
    from ttscube_amd.networks.textcoder_train import BnTanhDropoutFn
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(4, 512, 64, generator=gen).cuda()
    g, b = torch.ones(512).cuda(), torch.zeros(512).cuda() + 0.05
    dy = torch.randn(4, 512, 64, generator=gen).cuda()
    outs = []
    for mask in (None, 'from_y'):
        xg = x.clone().requires_grad_(True)
        m = None if mask is None else (outs[0][0] != 0).float()
        y = BnTanhDropoutFn.apply(xg, g, b, torch.zeros(512).cuda(), torch.ones(512).cuda(), m, 1234, 2, 0.1, 1e-5, 0.1)
        y.backward(dy)
        outs.append((y.detach(), xg.grad.detach()))
    keep = float((outs[0][0] != 0).float().mean())
    assert 0.88 < keep < 0.92, keep
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])   # the backward drew the forward's mask
    y2 = BnTanhDropoutFn.apply(x, g, b, torch.zeros(512).cuda(), torch.ones(512).cuda(), None, 1235, 2, 0.1, 1e-5, 0.1)
    assert not torch.equal(outs[0][0], y2)        # another seed, another mask


def _loss_ref(pd, td, pp, tp, pre, post, tm, ignore):
    ts = [t.detach().cpu().double().requires_grad_(True) for t in (pd, pp, pre, post)]
    ld = F.cross_entropy(ts[0], td.cpu(), ignore_index=ignore)
    lp = F.cross_entropy(ts[1], tp.cpu(), ignore_index=ignore)
    l1 = F.l1_loss(ts[2], tm.cpu().double())
    l2 = F.l1_loss(ts[3], tm.cpu().double())
    return [ld, lp, l1, l2], ts


def test_loss_kernel_matches_float64_torch_and_reports_bad_targets():
    from ttscube_amd import _lib
    from ttscube_amd.networks.textcoder_train import TextcoderLossFn, textcoder_losses
    gen = torch.Generator().manual_seed(9)
    Kd, Kp, ignore = 10, 201, 201          # ignore_index >= both class counts
    pd = torch.randn(3, 14, Kd, generator=gen).cuda()
    pp = torch.randn(3, 9, Kp, generator=gen).cuda() * 3
    td = torch.randint(0, Kd, (3, 14), generator=gen)
    td[1, 10:] = ignore
    td[2, :] = ignore                       # a whole utterance of ignored rows
    tp = torch.randint(0, Kp, (3, 9), generator=gen)
    tp[0, 5:] = ignore
    pre, post = torch.randn(3, 27, 80, generator=gen).cuda(), torch.randn(3, 27, 80, generator=gen).cuda()
    tm = torch.randn(3, 27, 80, generator=gen).cuda()
    args = (pd.reshape(-1, Kd), pp.reshape(-1, Kp), pre, post, td.reshape(-1).cuda(), tp.reshape(-1).cuda(), tm, ignore)
    ins = [a.clone().requires_grad_(True) for a in args[:4]]
    vals, status = TextcoderLossFn.apply(*ins, *args[4:])
    (vals * torch.tensor([1.0, 2.0, 3.0, 0.5], device='cuda')).sum().backward()
    assert int(status.item()) == 0
    ref, ts = _loss_ref(args[0], args[4], args[1], args[5], pre, post, tm, ignore)
    (ref[0] * 1 + ref[1] * 2 + ref[2] * 3 + ref[3] * 0.5).backward()
    for k in range(4):
        assert abs(float(vals[k]) - float(ref[k])) <= 1e-5 * max(1.0, abs(float(ref[k]))), k
    for a, t in zip(ins, ts):
        assert _rel(a.grad.cpu(), t.grad) <= 1e-5
    # every pitch row ignored: NaN loss and zero gradients, as torch's mean reduction gives
    tp_all = torch.full((27,), ignore, dtype=torch.long)
    v2, _ = TextcoderLossFn.apply(args[0], args[1][:27], pre, post, args[4], tp_all.cuda(), tm, ignore)
    assert np.isnan(float(v2[1])) and np.isnan(float(F.cross_entropy(args[1][:27].cpu(), tp_all, ignore_index=ignore)))
    # an out-of-range target that is not ignore_index: TTSCError from the status word, no device assert, and the process goes on
    bad = td.clone()
    bad[0, 3] = Kd + 2
    with pytest.raises(_lib.TTSCError, match='duration'):
        textcoder_losses(pd, pp, pre, post, bad.cuda(), tp.cuda(), tm, ignore, check=True)
    bad_p = tp.clone()
    bad_p[1, 0] = -3
    with pytest.raises(_lib.TTSCError, match='pitch'):
        textcoder_losses(pd, pp, pre, post, td.cuda(), bad_p.cuda(), tm, ignore, check=True)
    l_dur, l_pitch, l_mel, st = textcoder_losses(pd, pp, pre, post, td.cuda(), tp.cuda(), tm, ignore, check=True)
    assert int(st.item()) == 0 and abs(float(l_dur) - float(ref[0])) <= 1e-5 * max(1.0, float(ref[0]))
    assert abs(float(l_mel) - float(ref[2] + ref[3])) <= 1e-5 * max(1.0, float(ref[2] + ref[3]))


# ---- reference parity ---------------------------------------------------------------------------------------------------------------
class _Enc:
    def __init__(self, max_pitch, max_duration):
        self.phon2int = {'p%d' % i: i for i in range(40)}
        self.speaker2int = {'s%d' % i: i for i in range(2)}
        self.max_pitch, self.max_duration = max_pitch, max_duration


def _examples(z):
    out, o = [], 0
    for meta, n in zip(json.loads(str(z['ex_meta'])), z['ex_len']):
        n = int(n)
        out.append({'meta': meta, 'mgc': z['ex_mgc'][o:o + n], 'pitch': z['ex_pitch'][o:o + n]})
        o += n
    return out


def _golden_net(name):
    from ttscube_amd.io_utils.io_textcoder import TextcoderCollate
    from ttscube_amd.networks.textcoder import CubenetTextcoder
    z = np.load(os.path.join(ROOT, 'tests', 'golden', name + '.npz'))
    shapes = [(k, tuple(s)) for k, s in json.loads(str(z['shapes']))]
    cfg = json.loads(str(z['cfg']))
    enc = _Enc(cfg['max_pitch'], cfg['max_duration'])
    net = CubenetTextcoder(enc, pframes=int(z['pframes']))
    assert M.named_shapes(net) == shapes
    net.load_state_dict(M.fill_state_dict(shapes, int(z['seed'])), strict=True)
    batch = TextcoderCollate(enc).collate_fn(_examples(z))
    return z, net.cuda().train(), batch


def _masks(z, step):
    pre = np.unpackbits(z['mask%d_pre' % step], axis=-1)[..., :256].astype(np.float32)
    sh = z['mask%d_post_shape' % step]
    post = np.unpackbits(z['mask%d_post' % step], axis=-1)[..., :int(sh[-1])].astype(np.float32)
    return {'prenet': [torch.from_numpy(pre[0]).cuda(), torch.from_numpy(pre[1]).cuda()],
            'postnet': [torch.from_numpy(post[i]).cuda() for i in range(4)]}


# The bias of a convolution that feeds a training-mode BatchNorm has an exact gradient of ZERO (the batch mean removes it): the reference stores
# its round-off (norm ~1e-9 against ~0.2 for the weight), and Adam's scale-free first step turns any such noise into +-lr per element.  Those four
# tensors are held to "zero gradient" and "within 2 steps x 2 lr of the reference" instead; nothing downstream depends on them.
BN_FED_BIASES = ['_postnet.network.%d.conv.bias' % i for i in (0, 4, 8, 12)]


def _fp_bad(z, prefix, tensors, lr=2e-4):
    bad = {}
    for k in json.loads(str(z['grad_names'])):
        fp = {f: z['%s/%s/%s' % (prefix, k, f)] for f in ('norm', 'sum', 'probe', 'idx', 'samples', 'size')}
        if k in BN_FED_BIASES:
            t = tensors[k].detach().cpu().double().numpy().reshape(-1)
            w_norm = float(z['grad/%s/norm' % k.replace('bias', 'weight')])
            ok = (float(np.abs(t).max()) <= 1e-6 * w_norm and float(fp['norm']) <= 1e-6 * w_norm) if prefix == 'grad' else \
                float(np.abs(t[fp['idx']] - fp['samples']).max()) <= 4 * lr + 1e-6
            if not ok:
                bad[k] = 'BN-fed bias'
            continue
        dev = compare(tensors[k].detach().cpu().numpy(), k, fp)
        if max(dev.values()) > 1e-4:
            bad[k] = dev
    return bad


@pytest.mark.parametrize('name', ['textcoder_train_a', 'textcoder_train_b', 'textcoder_train_pf1'])
def test_textcoder_training_step_matches_the_reference(name, monkeypatch):
    from ttscube_amd.networks import textcoder_train as TT
    z, net, batch = _golden_net(name)
    seen = []
    orig = TT.textcoder_forward_train

    def spy(*a, **k):
        out = orig(*a, **k)
        seen.append(out)
        return out
    monkeypatch.setattr(TT, 'textcoder_forward_train', spy)
    out = net.training_step(batch, 0, dropout_masks=_masks(z, 0))
    p_dur, p_pitch, pre, post = seen[0]
    assert p_dur.requires_grad and post.requires_grad
    for got, key in ((p_dur, 'p_dur'), (p_pitch, 'p_pitch'), (pre, 'pre_mel'), (post, 'post_mel')):
        assert tuple(got.shape) == z[key].shape, key
        assert float((got.detach().cpu() - torch.from_numpy(z[key])).abs().max()) < 1e-4, key
    got_l = [out['loss'], out['l_mel'], out['l_pitch'], out['l_dur']]
    assert np.abs(np.asarray(got_l) - z['losses']).max() < 1e-4, (got_l, z['losses'])
    params = dict(net.named_parameters())
    assert not _fp_bad(z, 'grad', {k: p.grad for k, p in params.items()})
    sd = net.state_dict()
    for k in [k for k in z.files if k.startswith('bn/')]:
        assert _rel(sd[k[3:]].cpu(), z[k]) <= 1e-4, k
    net.training_step(batch, 1, dropout_masks=_masks(z, 1))['loss']
    assert not _fp_bad(z, 'param2', params)


def _run_steps(name, n, seed):
    z, net, batch = _golden_net(name)
    torch.manual_seed(seed)
    for i in range(n):
        net.training_step(batch, i)['loss']
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}, net, batch


def test_three_step_runs_are_bit_identical():
    a, _, _ = _run_steps('textcoder_train_b', 3, 77)
    b, _, _ = _run_steps('textcoder_train_b', 3, 77)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _postnet64(sd, x):
    """float64 eval-mode PostNet (modules.py:117-145): conv -> BatchNorm(running statistics) -> tanh, x 4, conv"""
    h = x.double().permute(0, 2, 1)
    for i in range(5):
        w, b = sd['_postnet.network.%d.conv.weight' % (4 * i)].double(), sd['_postnet.network.%d.conv.bias' % (4 * i)].double()
        h = F.conv1d(h, w, b, padding=2)
        if i < 4:
            p = '_postnet.network.%d.' % (4 * i + 1)
            h = torch.tanh(F.batch_norm(h, sd[p + 'running_mean'].double(), sd[p + 'running_var'].double(), sd[p + 'weight'].double(),
                                        sd[p + 'bias'].double(), training=False, eps=1e-5))
    return h.permute(0, 2, 1)


def test_eval_forward_after_training_uses_the_updated_running_statistics():
    sd0 = _golden_net('textcoder_train_b')[1].state_dict()
    rm0 = sd0['_postnet.network.1.running_mean'].cpu().clone()
    sd, net, batch = _run_steps('textcoder_train_b', 3, 5)
    assert not torch.equal(sd['_postnet.network.1.running_mean'], rm0)
    assert int(sd['_postnet.network.1.num_batches_tracked']) == 100 + 3
    net.eval()
    with torch.no_grad():
        _, _, mel, post = net(batch)            # the existing inference path: folded BatchNorm, no dropout
    ref = mel.cpu().double() + _postnet64(sd, mel.cpu())
    assert float((post.cpu().double() - ref).abs().max()) < 1e-4


def test_trainer_script_trains_saves_and_resumes(tmp_path):
    base = str(tmp_path / 'tc')
    cmd = [sys.executable, os.path.join(ROOT, 'scripts', 'train_textcoder.py'), '--synthetic', '8', '--epochs', '1', '--batch-size', '4',
           '--num-workers', '1', '--output-base', base]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    for ext in ('.yaml', '.encodings', '.best', '.last', '.opt.last'):
        assert os.path.exists(base + ext), ext
    shutil.copy(base + '.opt.last', base + '.opt.first')
    first = torch.load(base + '.opt.first', map_location='cpu')
    r = subprocess.run(cmd + ['--resume'], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'Resuming' in r.stdout
    second = torch.load(base + '.opt.last', map_location='cpu')
    s1 = {int(float(e['step'])) for e in first['state'].values()}
    s2 = {int(float(e['step'])) for e in second['state'].values()}
    assert s1 == {2} and s2 == {4}, (s1, s2)        # 8 items / batch 4 = 2 steps per epoch, continued from the saved state
    # the resumed optimizer holds exactly the saved state before its first update
    from ttscube_amd.io_utils.io_textcoder import TextcoderEncodings
    from ttscube_amd.networks.textcoder import CubenetTextcoder
    enc = TextcoderEncodings(base + '.encodings')
    net = CubenetTextcoder(enc)
    net.load(base + '.last')
    net._loaded_optimizer_state = first
    net = net.cuda()
    opt = net.optimizers()
    for p in net.parameters():
        p.grad = torch.zeros_like(p)
    opt.ensure_built()             # (lays the arenas out and applies the queued state)
    st = opt.state_dict()
    assert sorted(st['state']) == sorted(first['state'])
    for i, e in first['state'].items():
        assert torch.equal(st['state'][i]['exp_avg'].cpu(), e['exp_avg']) and torch.equal(st['state'][i]['exp_avg_sq'].cpu(), e['exp_avg_sq'])
        assert float(st['state'][i]['step']) == float(e['step'])
