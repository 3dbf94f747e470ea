"""Time the view-dependent texture (profiles/texture_sh.md).

    python tools/shtex_probe.py [--reps 9] [--texels 1048576] [--dirs 2] [--grid 354] [--cell 8] [--bake_grid 128] [--bake_reps 3]

Kernels.  ops.shtex_weights and ops.shtex_fit (degrees 0, 1, 2) on `texels` texels with random unit normals and colours and the
directions of tesselation `dirs`; ops.shtex_shade (degrees 0, 1, 2) on a 1080 x 1920 view of tools/atlas_probe.py's height field
of `grid`^2 squares with an atlas of `cell` texels.  Each is the median HIP-event time over `reps` calls after two untimed ones.
Bytes are the algorithm's: weights writes 4 B a pair; the fit reads 12 B a pair, of which the half with weight 0 is never loaded, (both
counts are given), and writes 12 K B a texel; the shading pass reads face, bary, three vertices, three UVs and four texels of 12 K B
a shaded pixel and writes 12 B.  The yardstick is a device-to-device copy of the fit's colour array (bytes = read + written).

End to end.  The height field of `bake_grid`^2 squares is baked from a model with random weights (the blender_refnerf preset at
full width) with and without sh_degree=2, alternating, host clock around calls that end in a device synchronise; the seconds inside
the colour function (the MLP) and inside the three ops are HIP-event sums over one further bake of each kind.  Prints one JSON line.

    python tools/shtex_probe.py bake_sphere CHECKPOINT_DIR OUT.ply [--bands 48] [--cell 8] [--degree 2]

bakes the unit sphere of the `procedural` scene from a blender_refnerf checkpoint for eval_mesh.py (see `bake_sphere`).
"""

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from atlas_probe import event_ms, height_field, host_s, parts_ms  # noqa: E402


def bake_sphere(checkpoint_dir, out, bands, cell, degree):
  """Bake the unit sphere (the surface of the `procedural` scene; a latitude-longitude mesh of `bands` bands) from the blender_refnerf
  checkpoint in `checkpoint_dir`, with sh_degree=`degree`, and write it as `out` (PLY + PNG + _sh.npy) for eval_mesh.py: the texture
  alone is under test, the geometry is exact."""
  from multinerf_amd import checkpoints, configs, mesh, train_utils
  config = configs.load_preset('blender_refnerf', ["Config.dataset_loader = 'procedural'", f"Config.checkpoint_dir = '{checkpoint_dir}'"])
  model, state, _, _, _ = train_utils.setup_model(config, 20200823, dataset=None, device=torch.device('cuda', 0))
  state = checkpoints.restore_checkpoint(checkpoint_dir, model, state)
  th, ph = np.pi * np.arange(1, bands) / bands, 2 * np.pi * np.arange(2 * bands) / (2 * bands)
  ring = np.stack([np.sin(th)[:, None] * np.cos(ph), np.sin(th)[:, None] * np.sin(ph), np.cos(th)[:, None] * np.ones_like(ph)], -1)
  v = np.concatenate([[[0, 0, 1.]], ring.reshape(-1, 3), [[0, 0, -1.]]]).astype(np.float32)
  at = lambda i, j: 1 + i * 2 * bands + (j % (2 * bands))
  f = []
  for j in range(2 * bands):
    f.append((0, at(0, j), at(0, j + 1)))
    for i in range(bands - 2):
      f += [(at(i, j), at(i + 1, j), at(i + 1, j + 1)), (at(i, j), at(i + 1, j + 1), at(i, j + 1))]
    f.append((len(v) - 1, at(bands - 2, j + 1), at(bands - 2, j)))
  m = dict(vertices=torch.from_numpy(v).cuda(), normals=torch.from_numpy(v).cuda(), faces=torch.tensor(f, dtype=torch.int32).cuda())
  baked = mesh.bake_texture(m, model=model, cell=cell, sh_degree=degree)
  os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
  mesh.write_ply(out, m, texture=baked)
  print(f'{out}: step {int(state.step)}, {len(f)} faces, atlas {baked["layout"]["W"]} x {baked["layout"]["H"]}, {baked["sh_queries"]} colour queries')
  own = baked['texture'][baked['mask'] == 255].to(torch.float32) / 255.
  print(f'texture: mean rgb {[round(float(c), 4) for c in own.mean(0)]}, std {[round(float(c), 4) for c in own.std(0)]}, '
        f'{float((own.max(-1).values < 0.05).float().mean()):.2%} of the texels below 0.05, {float((own.min(-1).values > 0.95).float().mean()):.2%} above 0.95')


def main():
  if len(sys.argv) > 1 and sys.argv[1] == 'bake_sphere':
    ap = argparse.ArgumentParser()
    ap.add_argument('mode')
    ap.add_argument('checkpoint_dir')
    ap.add_argument('out')
    ap.add_argument('--bands', type=int, default=48)
    ap.add_argument('--cell', type=int, default=8)
    ap.add_argument('--degree', type=int, default=2)
    a = ap.parse_args()
    return bake_sphere(a.checkpoint_dir, a.out, a.bands, a.cell, a.degree)
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=9)
  ap.add_argument('--texels', type=int, default=1 << 20)
  ap.add_argument('--dirs', type=int, default=2)
  ap.add_argument('--grid', type=int, default=354)
  ap.add_argument('--cell', type=int, default=8)
  ap.add_argument('--bake_grid', type=int, default=128, help='0: the kernels only')
  ap.add_argument('--bake_reps', type=int, default=3)
  ap.add_argument('--chunk', type=int, default=1 << 18)
  args = ap.parse_args()
  from multinerf_amd import configs, mesh, models, ops
  out = dict(reps=args.reps, device=torch.cuda.get_device_name(0))
  gen = torch.Generator('cuda').manual_seed(0)
  dirs = torch.from_numpy(mesh.sh_directions(args.dirs)).cuda()
  D, n = int(dirs.shape[0]), args.texels

  # ---- weights and fit
  normals = torch.nn.functional.normalize(torch.randn((n, 3), device='cuda', generator=gen), dim=-1).contiguous()
  rgb = torch.rand((n, D, 3), device='cuda', generator=gen)
  ms, lo, hi = event_ms(lambda: ops.shtex_weights(dirs, normals), args.reps)
  seen = int((ops.shtex_weights(dirs, normals) > 0).sum())
  out['weights'] = dict(texels=n, dirs=D, pairs=n * D, pairs_seen=seen, ms=ms, ms_min=lo, ms_max=hi, bytes=4 * n * D + 12 * n, GBps=(4 * n * D + 12 * n) / ms / 1e6)
  dst = torch.empty_like(rgb)
  ms, lo, hi = event_ms(lambda: dst.copy_(rgb), args.reps)
  out['copy'] = dict(bytes=2 * rgb.numel() * 4, ms=ms, ms_min=lo, ms_max=hi, GBps=2 * rgb.numel() * 4 / ms / 1e6)
  del dst
  for degree in (0, 1, 2):
    K = (degree + 1) ** 2
    basis = torch.from_numpy(ops.sh_basis(dirs, degree)).cuda()
    ms, lo, hi = event_ms(lambda: ops.shtex_fit(dirs, normals, rgb, degree, 1e-3, basis=basis), args.reps)
    all_b, seen_b = 12 * n * D + 12 * n + 12 * K * n, 12 * seen + 12 * n + 12 * K * n
    out[f'fit{degree}'] = dict(ms=ms, ms_min=lo, ms_max=hi, bytes_all_pairs=all_b, bytes_seen_pairs=seen_b, GBps_all_pairs=all_b / ms / 1e6,
                               GBps_seen_pairs=seen_b / ms / 1e6, texels_per_s=n / ms * 1e3)
  del rgb, normals
  torch.cuda.empty_cache()

  # ---- shade
  m = height_field(args.grid)
  T = int(m['faces'].shape[0])
  lay = ops.atlas_layout(T, args.cell)
  uv = ops.atlas_uvs(m, lay)
  H, W = 1080, 1920
  eye = np.array([0.3, -1.6, 1.4])
  fwd = -eye / np.linalg.norm(eye)
  right = np.cross(fwd, [0., 0., 1.])
  right /= np.linalg.norm(right)
  c2w = np.stack([right, np.cross(right, fwd), -fwd, eye], -1)
  pixtocam = np.linalg.inv(np.array([[1400., 0, W / 2.], [0, 1400., H / 2.], [0, 0, 1.]]))
  P = mesh.world_to_pixel(pixtocam, c2w)
  vis = ops.raster_visibility(m, P, H, W, 0.05)
  base = ops.raster_shade(m, P, vis, 0.05)
  hit = int((base['face'] >= 0).sum())
  for degree in (0, 1, 2):
    K = (degree + 1) ** 2
    sh = torch.rand((lay['H'], lay['W'], K, 3), device='cuda', generator=gen)
    rgb = base['rgb'].clone()
    ms, lo, hi = event_ms(lambda: ops.shtex_shade(m, base['face'], base['bary'], uv, sh, eye, rgb), args.reps)
    moved = 16 * H * W + hit * (12 + 36 + 24 + 4 * 12 * K + 12)
    out[f'shade{degree}'] = dict(T=T, atlas=[lay['W'], lay['H']], image=[W, H], pixels_shaded=hit, ms=ms, ms_min=lo, ms_max=hi, bytes=moved, GBps=moved / ms / 1e6)
    del sh
  ms, lo, hi = event_ms(lambda: ops.raster_shade(m, P, vis, 0.05), args.reps)
  out['raster_shade_untextured'] = dict(ms=ms, ms_min=lo, ms_max=hi)
  del m, uv, vis, base
  torch.cuda.empty_cache()
  if args.bake_grid <= 0:
    print(json.dumps(out))
    return

  # ---- end to end: the bake with and without the SH fit, the same MLP behind both
  config = configs.load_preset('blender_refnerf', ["Config.dataset_loader = 'procedural'"])
  model, _ = models.construct_model(20200823, None, config, device='cuda')
  m = height_field(args.bake_grid)
  lay = ops.atlas_layout(int(m['faces'].shape[0]), args.cell)
  inner = mesh._model_color_fn(model)
  spent = dict(s=0., calls=0, rows=0)

  def color_fn(*a):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = inner(*a)
    e1.record()
    torch.cuda.synchronize()
    spent['s'] += e0.elapsed_time(e1) / 1e3
    spent['calls'] += 1
    spent['rows'] += int(a[0].shape[0])
    return r

  plain = lambda fn=inner: mesh.bake_texture(m, color_fn=fn, cell=args.cell, chunk=args.chunk)
  sh = lambda fn=inner: mesh.bake_texture(m, color_fn=fn, cell=args.cell, chunk=args.chunk, sh_degree=2, sh_dirs=args.dirs)
  plain()
  sh()
  tp, ts = [], []
  for _ in range(args.bake_reps):
    tp.append(host_s(plain))
    ts.append(host_s(sh))
  stat = lambda t: dict(s_median=float(np.median(t)), s_min=min(t), s_max=max(t))
  out['bake_plain'] = dict(T=int(m['faces'].shape[0]), n_samples=lay['n_samples'], chunk=args.chunk, **stat(tp))
  out['bake_sh'] = dict(degree=2, dirs=D, **stat(ts))
  plain(color_fn)
  out['bake_plain'].update(colour_query_s=spent['s'], colour_calls=spent['calls'], colour_rows=spent['rows'])
  spent.update(s=0., calls=0, rows=0)
  parts = parts_ms(lambda: sh(color_fn), ['shtex_weights', 'shtex_fit', 'atlas_samples', 'atlas_store'])
  out['bake_sh'].update(colour_query_s=spent['s'], colour_calls=spent['calls'], colour_rows=spent['rows'], parts_ms=parts)
  print(json.dumps(out))


if __name__ == '__main__':
  main()
