"""The public HiFi-GAN trainer around the kernels this package already has: `hifigan_training_step` (the generator / discriminator part of
networks/training.py::cubegan_training_step without the text side, conditioned on mel), the data feed (io_utils/segment_feed.py: a device-resident
corpus, one gather launch per batch), checkpoints in the public layout (`g_%08d` = {'generator'}, `do_%08d` = {'mpd', 'msd', 'optim_g', 'optim_d',
'steps', 'epoch'}, config.json beside them: what io_utils/runtime.py::load_generator_checkpoint reads) and a ragged validation pass.
scripts/train_hifigan.py is the command line.

Three input-feature families (`--input-features`):
    audio   the generator's own features, mel_spectrogram of the crop (upstream's default)
    mgc     the corpus's `<id>.mgc` rows (MelVocoder.melspectrogram: log10), scaled by ln 10 in the gather — what synthesize_devset feeds it
    gta     `<input_mels_dir>/<id>.npy`, [80, F] in the generator's domain (scripts/export_gta_mels.py): upstream's --fine_tuning

Single GPU.  Nothing here has a CPU path: a CPU tensor raises TTSCError."""
import glob
import json
import os
import re
import shutil
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

from .. import _lib
from ..io_utils import segment_feed as SF


# ---- the step ---------------------------------------------------------------------------------------------------------------------------------
def loss_fmax(h):
    """`fmax_for_loss`; null -> sampling_rate / 2"""
    v = h.get('fmax_for_loss')
    if v is None:
        sr = int(h['sampling_rate'])
        return sr // 2 if sr % 2 == 0 else sr / 2.0
    return v


def _mel_args(h, fmax):
    return int(h['n_fft']), int(h['num_mels']), int(h['sampling_rate']), int(h['hop_size']), int(h['win_size']), h['fmin'], fmax


def hifigan_training_step(generator, mpd, msd, opt_g, opt_d, y, mel_in, h):
    """One step of the public HiFi-GAN trainer: y [B, 1, L] (or [B, L]) target audio, mel_in [B, num_mels, T] generator input, h the config.
       1. generator forward, both signals trimmed to the shorter
       2. mel_spectrogram of both with fmax_for_loss
       3. D step on the detached output: MPD + MSD discriminator_loss, backward, opt_d.step()
       4. G step: 45 x L1(mel) + two feature_loss + two generator_loss with the discriminator parameters frozen for the pass, backward, opt_g.step()
    Every piece is the one cubegan_training_step uses (networks/training.py: same hooks, same order of launches, raw feature maps, AmaxPool reset,
    the device-side guard word in front of the generator's FlatAdamW launch); nothing is formulated anew here.
    -> {'loss_d', 'loss_g', 'loss_mel' (un-weighted), 'loss_mel_x45' (as it enters loss_g), 'lr'}; with FlatAdamW a training.StepLosses, read back when first looked at."""
    import itertools

    from ..io_utils.melspec import mel_spectrogram
    from ..networks import training as T
    from ..optim import FlatAdamW
    from .autograd import generator_forward_with_grad
    for t_ in itertools.chain((y, mel_in), itertools.islice(generator.parameters(), 1), itertools.islice(mpd.parameters(), 1),
                              itertools.islice(msd.parameters(), 1)):
        T._require_device(t_, 'hifigan_training_step')
    discriminator_loss, feature_loss, generator_loss = T._gan_loss_fns()
    mpd_f, msd_f = T._discriminator_fns(types.SimpleNamespace(_mpd=mpd, _msd=msd))
    dev = y.device
    lazy = T.STEP_LAZY and isinstance(opt_g, FlatAdamW)
    from .wbank import AmaxPool
    AmaxPool.of(dev).reset()
    rb = None
    if lazy:
        rb = T._StepReadback.of(dev)
        rb.words.zero_()
    margs = _mel_args(h, loss_fmax(h))
    if y.dim() == 2:
        y = y.unsqueeze(1)
    y_g_hat = generator_forward_with_grad(generator, mel_in.contiguous())
    m = min(y.shape[2], y_g_hat.shape[2])
    y, y_g_hat = y[:, :, :m], y_g_hat[:, :, :m]
    y_mel = mel_spectrogram(y.squeeze(1), *margs)
    y_g_hat_mel = mel_spectrogram(y_g_hat.squeeze(1), *margs)
    # discriminator step
    opt_d.zero_grad()
    y_df_hat_r, y_df_hat_g, _, _ = mpd_f(y, y_g_hat.detach(), False)
    loss_disc_f, _, _ = discriminator_loss(y_df_hat_r, y_df_hat_g)
    y_ds_hat_r, y_ds_hat_g, _, _ = msd_f(y, y_g_hat.detach(), False)
    loss_disc_s, _, _ = discriminator_loss(y_ds_hat_r, y_ds_hat_g)
    loss_disc_all = loss_disc_s + loss_disc_f
    loss_disc_all.backward()
    opt_d.step()
    # generator step
    opt_g.zero_grad()
    loss_mel = F.l1_loss(y_mel, y_g_hat_mel) * 45
    d_params = [p for p in itertools.chain(mpd.parameters(), msd.parameters()) if p.requires_grad]
    for p in d_params:
        p.requires_grad_(False)
    try:
        fm = 'raw' if (T.FMAP_RAW and all(getattr(f, 'accepts_raw', False) for f in (mpd_f, msd_f, feature_loss))) else True
        y_df_hat_r, y_df_hat_g, fmap_f_r, fmap_f_g = mpd_f(y, y_g_hat, fm)
        y_ds_hat_r, y_ds_hat_g, fmap_s_r, fmap_s_g = msd_f(y, y_g_hat, fm)
        loss_gen_all = (generator_loss(y_ds_hat_g)[0] + generator_loss(y_df_hat_g)[0] + feature_loss(fmap_s_r, fmap_s_g)
                        + feature_loss(fmap_f_r, fmap_f_g) + loss_mel)
        loss_gen_all.backward()
    finally:
        for p in d_params:
            p.requires_grad_(True)
    lr = opt_g.param_groups[0]['lr']
    if lazy:
        rb.collect(0)
        opt_g.step(guard=rb.words[0:1])
        rb.collect(2, with_gemm=True)
        # (the read-back slot holds four losses in front of the status words: the fourth is the mel term as it enters loss_g)
        res = rb.send([loss_gen_all, loss_disc_all, loss_mel, loss_mel], {'_names': ('loss_g', 'loss_d', 'loss_mel', 'loss_mel_x45'), 'lr': lr})
        res.also(lambda d: {'loss_mel': d['loss_mel'] / 45})
        return res
    _lib.check_split_status('hifigan_training_step (before the generator update)', stream=_lib.current_stream().value or 0)
    opt_g.step()
    vals = torch.stack([loss_gen_all.detach(), loss_disc_all.detach(), loss_mel.detach()]).tolist()
    return {'loss_g': vals[0], 'loss_d': vals[1], 'loss_mel': vals[2] / 45, 'loss_mel_x45': vals[2], 'lr': lr}


# ---- files --------------------------------------------------------------------------------------------------------------------------------------
def parse_filelist(path):
    """the public trainer's lists: one `name|text` line per utterance (the text is optional) -> names"""
    names = []
    for line in open(path, encoding='utf-8'):
        line = line.strip()
        if line:
            names.append(line.split('|')[0].strip())
    return names


def discover_processed(folder, need_mgc=False):
    """`<folder>/train` and `<folder>/dev` as every other trainer here reads them -> ({id: wav path} train, dev): every `<id>.wav` (with need_mgc,
    only those beside an `<id>.mgc`), sorted"""
    out = []
    for part in ('train', 'dev'):
        base = os.path.join(folder, part)
        if not os.path.isdir(base):
            raise FileNotFoundError('%s does not exist' % base)
        ids = sorted(f[:-4] for f in os.listdir(base) if f.endswith('.wav') and (not need_mgc or os.path.exists(os.path.join(base, f[:-4] + '.mgc'))))
        out.append([(i, os.path.join(base, i + '.wav')) for i in ids])
    return out[0], out[1]


def scan_checkpoints(path):
    """-> (steps, g path, do path) of the latest PAIR `g_%08d` / `do_%08d` under path, or None.  A generator file without its `do_` twin (or the
    other way round: a save cut short) is passed over."""
    found = {}
    for pre in ('g_', 'do_'):
        for f in glob.glob(os.path.join(path, pre + '*')):
            m = re.fullmatch(re.escape(pre) + r'(\d{8})', os.path.basename(f))
            if m:
                found.setdefault(int(m.group(1)), {})[pre] = f
    pairs = [s for s, d in found.items() if len(d) == 2]
    if not pairs:
        return None
    s = max(pairs)
    return s, found[s]['g_'], found[s]['do_']


def save_generator(path, generator):
    """`g_%08d`: {'generator': state_dict with weight_g / weight_v}"""
    torch.save({'generator': {k: v.detach().cpu().clone() for k, v in generator.state_dict().items()}}, path)


def save_checkpoint(folder, steps, epoch, generator, mpd, msd, opt_g, opt_d):
    cpu = lambda sd: {k: (v.detach().cpu().clone() if torch.is_tensor(v) else v) for k, v in sd.items()}
    save_generator(os.path.join(folder, 'g_%08d' % steps), generator)
    torch.save({'mpd': cpu(mpd.state_dict()), 'msd': cpu(msd.state_dict()), 'optim_g': opt_g.state_dict(), 'optim_d': opt_d.state_dict(),
                'steps': int(steps), 'epoch': int(epoch)}, os.path.join(folder, 'do_%08d' % steps))


def read_wav_int16(path, sampling_rate):
    """the file's samples as int16 (mono; float files are scaled by 32767), refusing another rate as upstream does"""
    import scipy.io.wavfile
    rate, x = scipy.io.wavfile.read(path)
    if rate != sampling_rate:
        raise ValueError('%s: %d Hz, the config says %d' % (path, rate, sampling_rate))
    if x.ndim > 1:
        x = x.mean(axis=1)
    if x.dtype == np.int16:
        return np.ascontiguousarray(x)
    if x.dtype == np.int32:
        return (x >> 16).astype(np.int16)
    if x.dtype == np.uint8:
        return ((x.astype(np.int16) - 128) << 8).astype(np.int16)
    return np.asarray(np.clip(x, -1.0, 1.0) * 32767, dtype=np.int16)


def load_items(entries, features, sampling_rate, n_mels, mels_dir=None):
    """entries [(id, wav path)] -> SegmentCorpus items [(int16 audio, frame-major float32 mel or None)]"""
    items = []
    for name, wav in entries:
        a = read_wav_int16(wav, sampling_rate)
        mel = None
        if features == 'mgc':
            mel = np.asarray(np.load(wav[:-4] + '.mgc'), dtype=np.float32)
        elif features == 'gta':
            mel = np.ascontiguousarray(np.asarray(np.load(os.path.join(mels_dir, name + '.npy')), dtype=np.float32).T)
        if mel is not None and (mel.ndim != 2 or mel.shape[1] != n_mels):
            raise ValueError('%s: features of shape %s, [frames, %d] expected' % (name, mel.shape, n_mels))
        items.append((a, mel))
    return items


# ---- validation ---------------------------------------------------------------------------------------------------------------------------------
def input_mel(y, mel, h, features):
    """the generator's input for a gathered batch: the gathered rows, or (audio) mel_spectrogram of the gathered signal"""
    if features != 'audio':
        return mel
    from ..io_utils.melspec import mel_spectrogram
    with torch.no_grad():
        return mel_spectrogram(y.squeeze(1), *_mel_args(h, h.get('fmax'))).contiguous()


def validate(generator, corpus, h, features, batch=4):
    """Whole dev utterances through Generator inference in ragged batches -> mean over the items of the L1 between the two mel_spectrograms (with
    fmax_for_loss) over each item's OWN samples: padding never enters.  Not hot."""
    from ..io_utils.melspec import mel_spectrogram
    hop = corpus.hop
    margs = _mel_args(h, loss_fmax(h))
    scale = SF.LN10 if features == 'mgc' else 1.0
    was_training = generator.training
    generator.eval()
    errs = []
    try:
        with torch.no_grad():
            usable = [u for u in range(corpus.num) if min(int(corpus.n_frames[u]), int(corpus.length[u]) // hop) * hop > int(h['n_fft'])]
            for s in range(0, len(usable), batch):
                us = usable[s:s + batch]
                fr = [min(int(corpus.n_frames[u]), int(corpus.length[u]) // hop) for u in us]
                y, mel = corpus.gather(us, [0] * len(us), max(fr), mel_scale=scale)
                if features == 'audio':      # each item's own features: a padded row's last frames would see zeros where the item alone sees its reflection
                    mel = torch.full((len(us), int(h['num_mels']), max(fr)), SF.MEL_PAD, device=y.device)
                    for i, f in enumerate(fr):
                        mel[i, :, :f] = mel_spectrogram(y[i, :, :f * hop], *_mel_args(h, h.get('fmax')))
                y_hat = generator(mel.contiguous(), frames=fr)
                for i, f in enumerate(fr):
                    m = min(f * hop, generator.out_len(f))
                    a = mel_spectrogram(y[i, :, :m], *margs)
                    b = mel_spectrogram(y_hat[i, :, :m], *margs)
                    errs.append(F.l1_loss(a, b))
    finally:
        generator.train(was_training)
    if not errs:
        raise _lib.TTSCError('validate: no dev utterance is longer than one analysis window (%d samples)' % int(h['n_fft']))
    return float(torch.stack(errs).mean())


# ---- the trainer --------------------------------------------------------------------------------------------------------------------------------
def epoch_lr(h, epoch):
    """upstream's ExponentialLR stepped once per epoch, stated from the epoch number alone (a resumed run gets the same float)"""
    return float(h['learning_rate']) * float(h['lr_decay']) ** int(epoch)


def train(a, out=sys.stdout):
    """a: the namespace of scripts/train_hifigan.py::parser()"""
    from ..optim import FlatAdamW
    from .discriminators import MultiPeriodDiscriminator, MultiScaleDiscriminator
    from .env import AttrDict
    from .models import Generator
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        raise SystemExit('train_hifigan.py trains on one process: the multi-GPU exchange is not built for this trainer')
    _lib.require_gpu()
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    h = AttrDict(json.loads(open(a.config).read()))
    os.makedirs(a.checkpoint_path, exist_ok=True)
    cfg_copy = os.path.join(a.checkpoint_path, 'config.json')
    if os.path.abspath(a.config) != os.path.abspath(cfg_copy):
        shutil.copyfile(a.config, cfg_copy)
    features = 'gta' if a.fine_tuning else a.input_features
    if features == 'gta' and not a.input_mels_dir:
        raise SystemExit('--fine_tuning / --input-features gta read <input_mels_dir>/<id>.npy: pass --input_mels_dir')
    if a.processed_folder:
        train_e, dev_e = discover_processed(a.processed_folder, need_mgc=(features == 'mgc'))
    else:
        if not (a.input_training_file and a.input_validation_file):
            raise SystemExit('pass --input_training_file and --input_validation_file, or --processed-folder')
        train_e, dev_e = ([(n, os.path.join(a.input_wavs_dir, n + '.wav')) for n in parse_filelist(f)]
                          for f in (a.input_training_file, a.input_validation_file))
    if not train_e or not dev_e:
        raise SystemExit('no training or no validation utterances')
    sr, hop, n_mels = int(h['sampling_rate']), int(h['hop_size']), int(h['num_mels'])
    frames = int(h['segment_size']) // hop
    if frames < 1 or int(h['segment_size']) % hop:
        raise SystemExit('segment_size=%s is not a multiple of hop_size=%d' % (h['segment_size'], hop))
    B = int(h['batch_size'])
    corpus = SF.SegmentCorpus(load_items(train_e, features, sr, n_mels, a.input_mels_dir), hop, n_mels, dev)
    dev_corpus = SF.SegmentCorpus(load_items(dev_e, features, sr, n_mels, a.input_mels_dir), hop, n_mels, dev)
    spe = corpus.num // B
    if spe < 1:
        raise SystemExit('%d training utterances do not fill one batch of %d' % (corpus.num, B))
    out.write('Training files: %d\nValidation files: %d\ninput features: %s, %d frames per segment, %d steps per epoch\n'
              % (corpus.num, dev_corpus.num, features, frames, spe))

    seed = int(h.get('seed', 1234))
    torch.manual_seed(seed)
    torch.cuda.manual_seed(seed)
    generator, mpd, msd = Generator(h), MultiPeriodDiscriminator(), MultiScaleDiscriminator()
    steps, state = 0, None
    last = scan_checkpoints(a.checkpoint_path)
    if last is not None:
        steps, g_path, do_path = last
        out.write('Resuming from %s / %s\n' % (g_path, do_path))
        generator.load_state_dict(torch.load(g_path, map_location='cpu')['generator'])
        state = torch.load(do_path, map_location='cpu')
        mpd.load_state_dict(state['mpd'])
        msd.load_state_dict(state['msd'])
        steps = int(state['steps'])
    generator, mpd, msd = generator.to(dev).train(), mpd.to(dev).train(), msd.to(dev).train()
    betas = (float(h['adam_b1']), float(h['adam_b2']))
    opt_g = FlatAdamW(list(generator.parameters()), float(h['learning_rate']), betas=betas)
    opt_d = FlatAdamW(list(msd.parameters()) + list(mpd.parameters()), float(h['learning_rate']), betas=betas)
    if state is not None:
        opt_g.load_state_dict(state['optim_g'])
        opt_d.load_state_dict(state['optim_d'])
    scale = SF.LN10 if features == 'mgc' else 1.0
    saved_at = steps if last is not None else -1
    log = open(os.path.join(a.checkpoint_path, 'validation.log'), 'a')
    prev = None

    def report(p):
        s_, e_, res = p
        out.write('Steps : %d, epoch %d, Gen Loss Total : %.3f, Disc Loss : %.3f, Mel-Spec. Error : %.3f, lr %.3e\n'
                  % (s_, e_, res['loss_g'], res['loss_d'], res['loss_mel'], res['lr']))

    for epoch in range(steps // spe, int(a.training_epochs)):
        for o in (opt_g, opt_d):
            o.param_groups[0]['lr'] = epoch_lr(h, epoch)
        for utt, start in SF.epoch_batches(seed, epoch, corpus.n_frames, frames, B, first=steps % spe if epoch == steps // spe else 0):
            y, mel = corpus.gather(utt, start, frames, mel_scale=scale)
            res = hifigan_training_step(generator, mpd, msd, opt_g, opt_d, y, input_mel(y, mel, h, features), h)
            steps += 1
            if prev is not None:               # (read back after the next step has been queued: the host never waits for the GPU here)
                report(prev)
            prev = (steps, epoch, res) if steps % int(a.stdout_interval) == 0 else None
            if steps % int(a.checkpoint_interval) == 0:
                save_checkpoint(a.checkpoint_path, steps, steps // spe, generator, mpd, msd, opt_g, opt_d)
                saved_at = steps
            if steps % int(a.validation_interval) == 0:
                err = validate(generator, dev_corpus, h, features)
                line = 'steps %d  validation mel error %.6f' % (steps, err)
                out.write(line + '\n')
                log.write(line + '\n')
                log.flush()
    if prev is not None:
        report(prev)
    if steps and saved_at != steps:
        save_checkpoint(a.checkpoint_path, steps, steps // spe, generator, mpd, msd, opt_g, opt_d)
    log.close()
    out.flush()
    return steps
