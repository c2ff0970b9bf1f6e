"""Import a folder of Montreal Forced Aligner output (`<name>.wav` + `<name>.TextGrid`) into the processed corpus the trainers read:
`<output-folder>/{train,dev}/<id>.{json,mgc,pitch,wav}`.  The flags of the reference's scripts/import_textgrid.py, plus --output-folder, --batch
(utterances per GPU call of the spectrogram and of the pitch tracker), --device and --gpu-resample (files that are not at --sample-rate are
converted by the HIP resampler instead of scipy on the host).

    python scripts/import_textgrid.py --input-folder aligned/ --speaker anna --prefix ANNA --dev-ratio 0.01
    python scripts/train_textcoder.py ...      # reads data/processed/{train,dev}"""
import optparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def main(argv=None):
    parser = optparse.OptionParser()
    parser.add_option('--input-folder', action='store', dest='input_folder', help='Folder with the aligned *.wav + *.TextGrid pairs')
    parser.add_option('--output-folder', action='store', dest='output_folder', default='data/processed',
                      help='Where train/ and dev/ are written (default=data/processed)')
    parser.add_option('--dev-ratio', type='float', dest='dev_ratio', default=0.001, help='Ratio between dev and train (default=0.001)')
    parser.add_option('--speaker', action='store', dest='speaker', default='none', help='What label to use for the speaker (default="none")')
    parser.add_option('--sample-rate', type='int', dest='sample_rate', default=24000,
                      help='Upsample or downsample data to this sample-rate (default=24000)')
    parser.add_option('--hop-size', type='int', dest='hop_size', default=240, help='Frame analysis hop-size (default=240)')
    parser.add_option('--prefix', dest='prefix', default='FILE', help='What prefix to use for the filenames')
    parser.add_option('--original-text', dest='original_text', help='Used to fetch context from')
    parser.add_option('--batch', type='int', dest='batch', default=32, help='Utterances per GPU call (default=32)')
    parser.add_option('--device', dest='device', default='cuda:0', help='Device of the spectrogram and the pitch tracker (default=cuda:0)')
    parser.add_option('--gpu-resample', action='store_true', dest='gpu_resample', default=False,
                      help='Bring the files to --sample-rate on the GPU (io_utils/resample.py) instead of with scipy on the host')
    params, _ = parser.parse_args(sys.argv[1:] if argv is None else argv)
    if not params.input_folder:
        parser.print_help()
        return 1
    if params.batch < 1:
        parser.error('--batch must be at least 1')
    from ttscube_amd.io_utils.corpus_import import import_dataset
    resampler = None
    if params.gpu_resample:
        from ttscube_amd.io_utils.resample import Resampler
        resampler = Resampler(params.device)
    import_dataset(params.input_folder, params.output_folder, dev_ratio=params.dev_ratio, speaker=params.speaker, sample_rate=params.sample_rate,
                   hop_size=params.hop_size, prefix=params.prefix, original_text=params.original_text, batch=params.batch, device=params.device,
                   resampler=resampler)
    return 0


if __name__ == '__main__':
    sys.exit(main())
