"""Golden vectors for the WaveRNN path, produced by the REFERENCE ITSELF (imported from /root/reference).

    python tools/gen_golden_wavernn.py [case ...]  ->  tests/golden/mulaw_lut.npy, mulaw_kat.npz, wavernn_*.npz

The reference's sampler (`Categorical(logits).sample()`, cube/networks/loss.py:227-230) draws
`E = empty_like(probs).exponential_(1)` per step from torch's global CPU generator and returns argmax(probs/E).
We run `WaveRNN._inference` UNPATCHED after torch.manual_seed(s), replay the same exponential stream after the same
seed, and check the replay explains every emitted sample before saving g = -log(E) as the injected Gumbel noise.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import ref_import  # noqa: E402

ref_import.setup()
from cube.networks.loss import MOLOutput, MULAWOutput, RAWOutput  # noqa: E402
from cube.networks.modules import WaveRNN  # noqa: E402
from cube.networks.vocoder import CubenetVocoder  # noqa: E402
from oracle import wavernn_ref as O  # noqa: E402  (synthetic weights/inputs only)

OUT = os.path.join(ROOT, 'tests', 'golden')


def gen_mulaw():
    m = MULAWOutput()
    lut = m.decode(torch.arange(256)).numpy().astype(np.float32)
    np.save(os.path.join(OUT, 'mulaw_lut.npy'), lut)
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(4096, generator=g) * 2 - 1).float()
    x = torch.cat([x, torch.tensor([1.0, 0.9, 0.0, -0.9, -1.0, 1e-5, -1e-5, 0.5, -0.5])])
    np.savez(os.path.join(OUT, 'mulaw_kat.npz'), x=x.numpy(), enc=m.encode(x).numpy(), enc_raw=RAWOutput().encode(x).numpy(),
             dec_raw=RAWOutput().decode(torch.arange(256).float()).numpy())
    print('mulaw lut', lut[[0, 1, 127, 128, 254, 255]])


def replay_sampler(net, X, seed):
    """Run the reference UNPATCHED after torch.manual_seed(seed), replay the exponential stream its sampler consumed, and
    check that a sampler computing argmax(probs / E) on the replayed E reproduces every sample.  -> (wav [B, L], E [B, L, 256])"""
    B = X['mel'].shape[0]
    torch.manual_seed(seed)
    wav = net._inference(dict(X))  # numpy [B, L, 1]
    wav = wav.reshape(B, -1)
    L = wav.shape[1]
    # replay the exponential stream the sampler consumed
    torch.manual_seed(seed)
    E = torch.stack([torch.empty(B, 256).exponential_(1) for _ in range(L)], dim=1)  # [B, L, 256]
    # verify the replay by re-running the reference with a sampler that consumes the replayed E
    fn = net._output_functions
    step = [0]
    orig = fn.sample

    def patched(y):
        probs = torch.softmax(y, dim=-1)
        q = probs / E[:, step[0]].unsqueeze(1)
        step[0] += 1
        return fn.decode(torch.argmax(q, dim=-1))

    fn.sample = patched
    wav2 = net._inference(dict(X)).reshape(B, -1)
    fn.sample = orig
    assert np.array_equal(wav, wav2), 'exponential-stream replay does not reproduce the reference samples'
    return wav, E


def run_case(name, H, N, use_lowres, B, T, seed, output='mulaw'):
    up = 240 if use_lowres else 24
    torch.manual_seed(0)
    net = WaveRNN(num_layers=N, layer_size=H, upsample=up, upsample_low=10, use_lowres=use_lowres, output=output)
    sd = O.synthetic_state_dict(H=H, num_layers=N, use_lowres=use_lowres, seed=seed)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    net.eval()
    mel, x_low = O.synthetic_inputs(B, T, seed=seed + 1)
    X = {'mel': torch.from_numpy(mel)}
    if use_lowres:
        X['x_low'] = torch.from_numpy(x_low)
    wav, E = replay_sampler(net, X, seed)
    L = wav.shape[1]
    fn = net._output_functions
    # teacher-forced logits: WaveRNN._train_forward on random audio (modules.py:505-539, shift as in 553-558)
    g = torch.Generator().manual_seed(seed + 2)
    audio = (torch.rand(B, L, generator=g) * 2 - 1).float()
    xin = torch.nn.functional.pad(audio[:, :-1], (1, 0), value=0)
    Xt = dict(X)
    Xt['x'] = xin
    with torch.no_grad():
        logits = net._train_forward(Xt).numpy()
        loss = float(fn.loss(torch.from_numpy(logits), audio))
    blob = dict(H=H, N=N, use_lowres=int(use_lowres), B=B, T=T, seed=seed, output=output, mel=mel, x_low=x_low,
                gumbel=(-torch.log(E)).numpy().astype(np.float32), wav=wav.astype(np.float32),
                idx=fn.encode(torch.from_numpy(wav)).numpy().astype(np.uint8), audio=audio.numpy(),
                logits_tf=logits.astype(np.float32), loss_tf=np.float32(loss))
    np.savez_compressed(os.path.join(OUT, name + '.npz'), **blob)
    print(name, 'L', L, 'wav rms', float(np.sqrt((wav ** 2).mean())), 'uniq idx', len(np.unique(blob['idx'])))


def run_case_continuous(name, H, N, use_lowres, B, T, seed, output):
    """MOL / Gaussian / Beta outputs (loss.py:35-215; 'mol' is the reference default, modules.py:398).  The reference draws
    uniforms / normals from torch's global CPU generator inside sample(); for 'mol' and 'gm' we replay that stream after the
    same seed, check that the replay reproduces every sample, and store the random TERMS the reference added:
      mol: 10 Gumbel terms -log(-log(u1)) + 1 logistic term log(u2) - log(1 - u2)   -> noise [B, L, 11]
      gm : z * 0.8                                                                   -> noise [B, L, 1]
    Beta sampling goes through torch's rejection sampler (not replayable): its golden holds the teacher-forced outputs and
    the loss only; the sampler is pinned distributionally in tests/test_oracle_wavernn.py."""
    up = 240 if use_lowres else 24
    S = O.SAMPLE_SIZE[output]
    torch.manual_seed(0)
    net = WaveRNN(num_layers=N, layer_size=H, upsample=up, upsample_low=10, use_lowres=use_lowres, output=output)
    sd = O.synthetic_state_dict(H=H, num_layers=N, use_lowres=use_lowres, seed=seed, S=S)
    if output == 'mol':     # keep the log-scales in a range where samples are not all clamped to +-1
        sd['_output.linear_layer.weight'][20:] *= 0.25
        sd['_output.linear_layer.bias'][20:] = sd['_output.linear_layer.bias'][20:] * 0.5 - 3.0
        sd['_output.linear_layer.weight'][10:20] *= 0.5
    if output == 'gm':
        sd['_output.linear_layer.weight'][1:] *= 0.25
        sd['_output.linear_layer.bias'][1:] -= 2.5
        sd['_output.linear_layer.weight'][:1] *= 0.3
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    net.eval()
    mel, x_low = O.synthetic_inputs(B, T, seed=seed + 1)
    X = {'mel': torch.from_numpy(mel)}
    if use_lowres:
        X['x_low'] = torch.from_numpy(x_low)
    fn = net._output_functions
    blob = dict(H=H, N=N, use_lowres=int(use_lowres), B=B, T=T, seed=seed, output=output, mel=mel, x_low=x_low,
                out_w=sd['_output.linear_layer.weight'], out_b=sd['_output.linear_layer.bias'])
    L = T * up
    if output in ('mol', 'gm'):
        torch.manual_seed(seed)
        wav = net._inference(dict(X)).reshape(B, -1)
        L = wav.shape[1]
        torch.manual_seed(seed)
        if output == 'mol':
            u1, u2 = [], []
            for _ in range(L):
                u1.append(torch.empty(B, 1, 10).uniform_(1e-5, 1 - 1e-5))
                u2.append(torch.empty(B, 1).uniform_(1e-5, 1.0 - 1e-5))
            u1, u2 = torch.cat(u1, dim=1), torch.cat(u2, dim=1)              # [B, L, 10], [B, L]
            noise = torch.cat([-torch.log(-torch.log(u1)), (torch.log(u2) - torch.log(1. - u2)).unsqueeze(2)], dim=2)
        else:
            noise = torch.cat([torch.randn((B, 1, 1)) * 0.8 for _ in range(L)], dim=1)   # [B, L, 1]
        step = [0]
        orig = fn.sample
        kidx = np.zeros((B, L), dtype=np.uint8)

        def patched(y, *a, **k):
            t = step[0]
            step[0] += 1
            if output == 'mol':
                temp = y[:, :, :10].data + noise[:, t, :10].unsqueeze(1)
                _, am = temp.max(dim=-1)
                kidx[:, t] = am[:, 0].numpy()
                oh = torch.nn.functional.one_hot(am, 10).float()
                means = torch.sum(y[:, :, 10:20] * oh, dim=-1)
                ls = torch.clamp(torch.sum(y[:, :, 20:30] * oh, dim=-1), min=float(np.log(1e-14)))
                x = means + torch.exp(ls) * noise[:, t, 10].unsqueeze(1)
                return torch.clamp(torch.clamp(x, min=-1.), max=1.)
            return (y[:, :, 0].unsqueeze(2) + noise[:, t].unsqueeze(1) * torch.exp(y[:, :, 1].unsqueeze(2))).squeeze(1)

        fn.sample = patched
        wav2 = net._inference(dict(X)).reshape(B, -1)
        fn.sample = orig
        assert np.array_equal(wav, wav2), 'random-stream replay does not reproduce the reference samples'
        blob.update(noise=noise.numpy().astype(np.float32), wav=wav.astype(np.float32), idx=kidx)
    g = torch.Generator().manual_seed(seed + 2)
    audio = (torch.rand(B, L, generator=g) * 1.6 - 0.8).float()
    xin = torch.nn.functional.pad(audio[:, :-1], (1, 0), value=0)
    Xt = dict(X)
    Xt['x'] = xin
    with torch.no_grad():
        logits = net._train_forward(Xt)
        loss = float(fn.loss(logits, audio))
    blob.update(audio=audio.numpy(), logits_tf=logits.numpy().astype(np.float32), loss_tf=np.float32(loss))
    np.savez_compressed(os.path.join(OUT, name + '.npz'), **blob)
    print(name, 'L', L, 'loss', loss, ('wav rms %.3f clamp share %.3f' % (float(np.sqrt((blob['wav'] ** 2).mean())),
                                                                        float((np.abs(blob['wav']) >= 1).mean()))) if 'wav' in blob else '')


DELTA = 1e-4        # near-tie threshold on the top-two gap of log_softmax(logits) + g (float64)
MIN_TIE = 4800      # the first near tie must not come before this step
LOG_EVERY = 100     # free-running logits stored at every LOG_EVERY-th step
T_TF = 1            # frames of the teacher-forced prefix (the full run's logits would be 24 MB)


def run_case_long(name, H, N, T, seed, noise_seed0):
    """One utterance over T frames (T * 240 steps) with noise generated from a stored seed (oracle.wavernn_ref.gumbel_from_seed)
    and injected into the reference's own sampler as E = exp(-g).  The first noise seed from noise_seed0 on whose run no
    near tie (top-two margin < DELTA) comes before MIN_TIE is kept; t_tie is the first near-tie step (L if none).  One torch
    thread: the run is B = 1 matrix-vector work, and the summation order of the reference's GEMVs stays fixed."""
    nthreads = torch.get_num_threads()
    torch.set_num_threads(1)
    torch.manual_seed(0)
    net = WaveRNN(num_layers=N, layer_size=H, upsample=240, upsample_low=10, use_lowres=True, output='mulaw')
    sd = O.synthetic_state_dict(H=H, num_layers=N, use_lowres=True, seed=seed)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    net.eval()
    mel, x_low = O.synthetic_inputs(1, T, seed=seed + 1)
    X = {'mel': torch.from_numpy(mel), 'x_low': torch.from_numpy(x_low)}
    # the probs / E sampler is the reference's Categorical sampler: proven on a two-frame prefix
    replay_sampler(net, {'mel': X['mel'][:, :2], 'x_low': X['x_low'][:, :48]}, seed)
    L = T * 240
    fn = net._output_functions
    orig = fn.sample
    for noise_seed in range(noise_seed0, noise_seed0 + 100):
        g = O.gumbel_from_seed(noise_seed, 1, L)
        g64 = torch.from_numpy(g.astype(np.float64))
        E = torch.exp(-torch.from_numpy(g))
        margin = np.zeros((1, L), dtype=np.float64)
        logits_fr = np.zeros((1, L // LOG_EVERY, 256), dtype=np.float32)
        step = [0]

        def patched(y):
            t = step[0]
            v = torch.log_softmax(y[:, 0].double(), dim=-1) + g64[:, t]
            top = torch.topk(v, 2, dim=-1).values
            margin[:, t] = (top[:, 0] - top[:, 1]).numpy()
            if t < MIN_TIE and margin[:, t].min() < DELTA:
                raise StopIteration(t)
            if t % LOG_EVERY == 0:
                logits_fr[:, t // LOG_EVERY] = y[:, 0].numpy()
            q = torch.softmax(y, dim=-1) / E[:, t].unsqueeze(1)
            step[0] += 1
            return fn.decode(torch.argmax(q, dim=-1))

        fn.sample = patched
        try:
            wav = net._inference(dict(X)).reshape(1, -1)
        except StopIteration as e:
            print(name, 'noise_seed', noise_seed, 'near tie at step', e.args[0], '< %d: next seed' % MIN_TIE)
            continue
        finally:
            fn.sample = orig
        break
    else:
        raise RuntimeError('no noise seed without a near tie before step %d' % MIN_TIE)
    assert wav.shape[1] == L
    below = np.flatnonzero(margin[0] < DELTA)
    t_tie = int(below[0]) if len(below) else L
    # teacher-forced logits on a T_TF-frame prefix
    Xt = {'mel': X['mel'][:, :T_TF], 'x_low': X['x_low'][:, :T_TF * 24]}
    Lt = T_TF * 240
    gen = torch.Generator().manual_seed(seed + 2)
    audio = (torch.rand(1, Lt, generator=gen) * 2 - 1).float()
    Xt['x'] = torch.nn.functional.pad(audio[:, :-1], (1, 0), value=0)
    with torch.no_grad():
        logits = net._train_forward(Xt).numpy()
        loss = float(fn.loss(torch.from_numpy(logits), audio))
    blob = dict(H=H, N=N, use_lowres=1, B=1, T=T, seed=seed, output='mulaw', mel=mel, x_low=x_low,
                noise_seed=noise_seed, noise_sha256=O.noise_sha256(g), delta=DELTA, t_tie=t_tie,
                margin=margin.astype(np.float32), wav=wav.astype(np.float32), idx=fn.encode(torch.from_numpy(wav)).numpy().astype(np.uint8),
                log_every=LOG_EVERY, logits_fr=logits_fr, T_tf=T_TF, audio=audio.numpy(), logits_tf=logits.astype(np.float32),
                loss_tf=np.float32(loss))
    path = os.path.join(OUT, name + '.npz')
    np.savez_compressed(path, **blob)
    torch.set_num_threads(nthreads)
    print(name, 'L', L, 'noise_seed', noise_seed, 't_tie', t_tie, 'min margin %.3g at step %d' % (margin.min(), int(margin.argmin())),
          'near ties', len(below), 'uniq idx', len(np.unique(blob['idx'])), 'bytes', os.path.getsize(path))


def gen_vocoder_fold():
    """CubenetVocoder._inference_batch / _compose_batched_inference shapes + values on T=40 (vocoder.py:109-131)."""
    torch.manual_seed(0)
    voc = CubenetVocoder(num_layers_lr=1, layer_size_lr=16, num_layers_hr=1, layer_size_hr=16, upsample=240,
                         upsample_low=10, output='mulaw')
    mel, _ = O.synthetic_inputs(1, 43, seed=77)
    x_low = np.random.RandomState(3).uniform(-1, 1, size=(1, 43 * 24)).astype(np.float32)
    fold = voc._inference_batch(torch.from_numpy(mel), torch.from_numpy(x_low), num_batches=20)
    hr = np.random.RandomState(4).uniform(-1, 1, size=(20, fold['x_low'].shape[1] * 10)).astype(np.float32)
    comp = voc._compose_batched_inference(hr)
    np.savez_compressed(os.path.join(OUT, 'vocoder_fold.npz'), mel=mel, x_low=x_low, fold_mel=fold['mel'].numpy(),
                        fold_x_low=fold['x_low'].numpy(), hr=hr, composed=comp)
    print('fold', tuple(fold['mel'].shape), tuple(fold['x_low'].shape), comp.shape)


CASES = {
    'mulaw': gen_mulaw,
    'vocoder_fold': gen_vocoder_fold,
    'wavernn_hr_h64_n1': lambda: run_case('wavernn_hr_h64_n1', 64, 1, True, 2, 2, 11),
    'wavernn_hr_h64_n2': lambda: run_case('wavernn_hr_h64_n2', 64, 2, True, 2, 1, 12),
    'wavernn_lr_h64_n1': lambda: run_case('wavernn_lr_h64_n1', 64, 1, False, 2, 6, 13),
    'wavernn_hr_h512_n1': lambda: run_case('wavernn_hr_h512_n1', 512, 1, True, 1, 1, 14),
    'wavernn_hr_h64_raw': lambda: run_case('wavernn_hr_h64_raw', 64, 1, True, 1, 1, 15, output='raw'),
    'wavernn_hr_h64_mol': lambda: run_case_continuous('wavernn_hr_h64_mol', 64, 1, True, 2, 2, 16, 'mol'),
    # the reference's default constructor arguments
    'wavernn_hr_h512_mol': lambda: run_case_continuous('wavernn_hr_h512_mol', 512, 2, True, 1, 1, 17, 'mol'),
    'wavernn_lr_h64_gm': lambda: run_case_continuous('wavernn_lr_h64_gm', 64, 1, False, 2, 5, 18, 'gm'),
    'wavernn_hr_h64_beta': lambda: run_case_continuous('wavernn_hr_h64_beta', 64, 1, True, 2, 1, 19, 'beta'),
    # 100 frames = 24 000 steps, noise from a stored seed (N = 2 is the reference class's default depth)
    'wavernn_hr_h512_n1_long': lambda: run_case_long('wavernn_hr_h512_n1_long', 512, 1, 100, 20, 1000),
    'wavernn_hr_h512_n2_long': lambda: run_case_long('wavernn_hr_h512_n2_long', 512, 2, 100, 21, 2000),
}

if __name__ == '__main__':
    # python tools/gen_golden_wavernn.py [case ...]   (no argument: every case)
    os.makedirs(OUT, exist_ok=True)
    for c in sys.argv[1:] or list(CASES):
        CASES[c]()
