"""`python -m dasr_amd.test -opt X.json` -- SRN inference / evaluation driver (reference: codes/SRN/test.py:17-138).

For every dataset of the option file: feed_data -> train.run_inference -> train.sr_and_scores -> SR image saved under
<results_root>/<dataset name>/imgs, and, when HR is present, PSNR / SSIM on the `scale`-pixel-cropped uint8 images in RGB and on the
Y channel, per image and averaged (same log lines as the reference).  `device_metrics: true` quantises the images and evaluates the four numbers on the
GPU (dasr_amd/metrics.py) instead of with util.host_scores on get_current_visuals; absent, the host path is unchanged.  `chop: true` runs the quadrant inference.  `self_ensemble: true` replaces test() by test_x8(), the x8 geometric self-ensemble (SR_model.py:102-140), everything downstream unchanged.  `back_projection: true | N` back-projects every SR image onto its LR image (20 | N iterations, dasr_amd/backproject.py) before it is saved and scored.  `val_lpips: true` adds the
LPIPS(alex) distance of the 8-bit images (test.py:88-128; weights from `path.lpips_alexnet` / `path.lpips_lin`, seeded when absent).
Every SR image goes to one png.FileWriter per dataset: PIL on this thread, or, under `device_png: true`, the quantised image stays on the device and the device PNG encoder writes it (dasr_amd/png.py); the pixels of the files are the same.
`save_RealorFake` needs the discriminator visual, not available here: NotImplementedError.  Datasets: `mode: "LRHR"` (HR folder, LR folder or LR made by bicubic down-sampling) and `mode: "LR"` read image folders through data.EvalFolderDataset; `mode: "synthetic"` ships
seeded LR/HR pairs; any iterable of the reference's batch dicts works through `main(loaders=...)`.
"""
import argparse
import logging
import os
import time
from collections import OrderedDict

from . import options as option
from . import png, util
from .models import create_model
from .train import BACK_PROJECTION_NOTE, DEVICE_PNG_NOTE, DEVICE_PNG_THREADS, SELF_ENSEMBLE_NOTE, create_dataset, run_inference, setup_logger, sr_and_scores


def evaluate(model, loader, opt, dataset_dir, logger, scale):
    # `device_png`: the device encoder; else PIL on this thread, inside write().  The files of this dataset are complete when the block is left
    with png.FileWriter(opt['device_png'], DEVICE_PNG_THREADS if opt['device_png'] else 0, note=None) as writer:
        return _evaluate(model, loader, opt, dataset_dir, logger, scale, writer)


def _evaluate(model, loader, opt, dataset_dir, logger, scale, writer):
    res = OrderedDict((k, []) for k in ('psnr', 'ssim', 'psnr_y', 'ssim_y', 'lpips'))
    for data in loader:
        need_HR = 'HR' in data
        model.feed_data(data, False)
        img_name = os.path.splitext(os.path.basename(data['LR_path'][0]))[0]
        run_inference(model, opt)
        sr_img, m, lpips = sr_and_scores(model, opt, need_HR, scale)   # `device_metrics`: quantised and scored on the GPU, the same bytes and numbers
        suffix = opt['suffix']
        writer.write(sr_img, os.path.join(dataset_dir, img_name + (suffix or '') + '.png'), 'bgr' if sr_img.ndim == 3 else 'grey')
        if not need_HR:
            logger.info(img_name)
            continue
        psnr, ssim = m['psnr'], m['ssim']
        res['psnr'].append(psnr)
        res['ssim'].append(ssim)
        if lpips is not None:      # test.py:88-100
            lpips = float(lpips)
            res['lpips'].append(lpips)
        if sr_img.ndim == 3 and sr_img.shape[2] == 3:
            psnr_y, ssim_y = m['psnr_y'], m['ssim_y']
            res['psnr_y'].append(psnr_y)
            res['ssim_y'].append(ssim_y)
            if lpips is not None:
                logger.info('{:20s} - PSNR: {:.6f} dB; SSIM: {:.6f}; PSNR_Y: {:.6f} dB; SSIM_Y: {:.6f}; {}: {:.3f}.'.format(img_name, psnr, ssim, psnr_y, ssim_y, model.lpips_label, lpips))
            else:
                logger.info('{:20s} - PSNR: {:.6f} dB; SSIM: {:.6f}; PSNR_Y: {:.6f} dB; SSIM_Y: {:.6f};.'.format(img_name, psnr, ssim, psnr_y, ssim_y))
        else:
            logger.info('{:20s} - PSNR: {:.6f} dB; SSIM: {:.6f}.'.format(img_name, psnr, ssim))
    return res


def main(argv=None, loaders=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('-opt', type=str, required=True, help='Path to options JSON file.')
    opt = option.parse(ap.parse_args(argv).opt, is_train=False)
    for key, path in opt['path'].items():
        if key != 'pretrain_model_G' and path:
            util.mkdir(path)
    opt = option.dict_to_nonedict(opt)
    if opt['save_RealorFake']:
        # codes/SRN/test.py:44,65-66,77: the patch map comes from visuals['realorfake'], which only DePatchGAN_wavelet_model.get_current_visuals
        # (DePatchGAN_wavelet_model.py:287-309, model 'De_patch_wavelet_GAN': the SRN tree's own copy of the DSN, outside SURVEY 8) produces; with the
        # trainers this path serves ('sr', 'DASR') the reference's test.py itself stops with KeyError at test.py:66.  The DSN's patch maps are written by
        # `python -m dasr_amd.dsn_create_dataset` (fake LR + domain-distance map, codes/DSN/create_dataset_modified.py).
        raise NotImplementedError("save_RealorFake needs model 'De_patch_wavelet_GAN' (its get_current_visuals is the only one with a 'realorfake' entry); "
                                  "use dasr_amd.dsn_create_dataset for the DSN's discriminator maps")
    setup_logger('base', opt['path']['log'], 'test', screen=True)
    logger = logging.getLogger('base')
    logger.info(option.dict2str(opt))
    if loaders is None:
        loaders = []
        for phase, ds in sorted(opt['datasets'].items()):
            ds['phase'] = 'test'
            loaders.append((ds['name'], create_dataset(ds, opt)))
    model = create_model(opt)
    if opt['self_ensemble']:
        logger.info(SELF_ENSEMBLE_NOTE)
    if option.back_projection_iters(opt['back_projection']):
        logger.info(BACK_PROJECTION_NOTE.format(option.back_projection_iters(opt['back_projection'])))
    if opt['device_png']:
        logger.info(DEVICE_PNG_NOTE)
    summary = OrderedDict()
    for name, loader in loaders:
        logger.info('\nTesting [{:s}]...'.format(name))
        t0 = time.time()
        dataset_dir = os.path.join(opt['path']['results_root'], name, 'imgs')
        util.mkdir(dataset_dir)
        res = evaluate(model, loader, opt, dataset_dir, logger, opt['scale'])
        if res['psnr']:
            ave_psnr, ave_ssim = sum(res['psnr']) / len(res['psnr']), sum(res['ssim']) / len(res['ssim'])
            summary[name] = {'psnr': ave_psnr, 'ssim': ave_ssim}
            if res['lpips']:
                summary[name]['lpips'] = sum(res['lpips']) / len(res['lpips'])
                logger.info('----Average PSNR/SSIM/{} results for {}----\n\tPSNR: {:.6f} dB; SSIM: {:.6f}; {}: {:.3f}\n'.format(
                    model.lpips_label, name, ave_psnr, ave_ssim, model.lpips_label, summary[name]['lpips']))
            else:
                logger.info('----Average PSNR/SSIM/LPIPS results for {}----\n\tPSNR: {:.6f} dB; SSIM: {:.6f}\n'.format(name, ave_psnr, ave_ssim))
            if res['psnr_y']:
                ay, asy = sum(res['psnr_y']) / len(res['psnr_y']), sum(res['ssim_y']) / len(res['ssim_y'])
                logger.info('----Y channel, average PSNR/SSIM----\n\tPSNR_Y: {:.6f} dB; SSIM_Y: {:.6f}\n'.format(ay, asy))
                summary[name].update(psnr_y=ay, ssim_y=asy)
        logger.info('[{:s}] done in {:.1f} s'.format(name, time.time() - t0))
    return summary


if __name__ == '__main__':
    main()
