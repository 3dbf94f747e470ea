"""train.py, eval.py and render.py with --preset llff_raw on the procedural raw capture (subprocesses, one GPU; nothing on
disk but the checkpoint directory), once with the quadratic colour correction and once with Config.eval_raw_affine_cc.  -m gpu."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(script, args, env):
  r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + args, capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
  print(r.stdout[-2500:], r.stderr[-2500:])
  assert r.returncode == 0, script
  return r.stdout


@pytest.mark.parametrize('affine', [False, True])
def test_llff_raw_train_eval_render(tmp_path, affine):
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  from PIL import Image
  ck = str(tmp_path / 'exp' / 'scene')
  binds = ["Config.dataset_loader = 'procedural'", 'Config.forward_facing = False', 'Config.near = 2.', 'Config.far = 6.',
           'Config.factor = 2', f"Config.checkpoint_dir = '{ck}'", 'Config.max_steps = 60', 'Config.batch_size = 2048',
           'Config.print_every = 20', 'Config.train_render_every = 60', 'Config.checkpoint_every = 30', 'Config.lr_delay_steps = 0',
           'NerfMLP.net_width = 128', 'PropMLP.net_width = 128', 'NerfMLP.bottleneck_width = 128', 'Config.eval_dataset_limit = 2',
           'Config.render_chunk_size = 4096']
  if affine:
    binds.append('Config.eval_raw_affine_cc = True')
  args = ['--preset', 'llff_raw']
  for b in binds:
    args += ['--gin_bindings', b]
  env = dict(os.environ, PYTHONPATH=ROOT)
  _run('train.py', args, env)
  log = [json.loads(l) for l in open(os.path.join(ck, 'train_log.jsonl'))]
  losses = [e['loss'] for e in log if 'loss' in e]
  assert len(losses) == 3 and losses[-1] < losses[0]
  assert any('test_psnr' in e for e in log)
  splits = {e['raw_split']: e for e in log if 'raw_split' in e}
  assert set(splits) == {'train', 'test'} and len(splits['train']['unique_shutters']) == 3
  assert len(splits['train']['exposure_idx']) == 40 and splits['test']['exposure_values'] == [1.0] * 6

  out = _run('eval.py', args, env)
  assert 'Evaluating checkpoint at step 60' in out and 'Average test psnr over 2 images' in out
  preds = os.path.join(ck, 'test_preds')
  assert os.path.exists(os.path.join(preds, 'metric_cc_psnr_60.txt'))
  # the saved images are post-processed: brighter than the raw-space rendering written as it is
  from multinerf_amd import checkpoints, configs, datasets, models, train_utils
  config = configs.load_preset('llff_raw', binds)
  dataset = datasets.load_dataset('test', None, config, device='cuda')
  model, state, render_eval_pfn, _, _ = train_utils.setup_model(config, 20200823, dataset=dataset, device='cuda')
  state = checkpoints.restore_checkpoint(ck, model, state)
  for idx, name in ((0, 'color_cc_000.png'), (1, 'color_001.png')):
    batch = dataset.generate_ray_batch(idx)
    rendering = models.render_image(lambda rng, r: render_eval_pfn(state.params, 1.0, None, r), batch.rays, None, config, verbose=False)
    raw_dark = float((rendering['rgb'].clamp(0, 1) * 255).to(torch.uint8).float().mean())
    saved = np.asarray(Image.open(os.path.join(preds, name)))
    print(f'{name}: mean 8-bit value {saved.mean():.2f}, of the raw-space rendering {raw_dark:.2f}')
    assert saved.shape == (48, 48, 3) and saved.mean() > raw_dark

  out = _run('render.py', args + ['--gin_bindings', 'Config.render_path = True', '--gin_bindings', 'Config.render_path_frames = 2'], env)
  assert 'Rendering checkpoint at step 60.' in out
  frames = os.path.join(ck, 'render', 'path_renders_step_60')
  files = set(os.listdir(frames))
  assert {'color_000.png', 'color_001.png', 'acc_001.tiff', 'distance_mean_000.tiff'} <= files, sorted(files)
  assert np.asarray(Image.open(os.path.join(frames, 'color_001.png'))).shape == (48, 48, 3)
  assert sorted(os.listdir(os.path.join(ck, 'render', 'scene_exp_path_renders_step_60_color'))) == ['000.png', '001.png']
