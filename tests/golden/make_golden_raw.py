#!/usr/bin/env python
"""Record the reference's own RawNeRF data path (internal/raw_utils.py).

    python tests/golden/make_golden_raw.py            # writes tests/golden/raw_utils.npz

The reference module is imported FROM WHERE IT LIES (MULTINERF_REFERENCE, nothing is copied) on the NumPy stand-in of
tests/golden/make_golden.py.  Stand-ins beyond those:

  * `jnp.array` and `jax.jit`-ed functions cast float64 input to float32, as jax does with x64 off: the demosaic and the
    downsample of load_raw_dataset then run in float32, the normalisation before them in NumPy float64;
  * a stub `rawpy` whose `imread(f).raw_image` is `np.load(f)`: the scenes are written to a temporary directory as files
    named `.dng` that hold `.npy` bytes, next to `.json` EXIF files;
  * `internal.utils` reduced to `file_exists`, `open_file` and `DataSplit`.

The .npz holds arrays only: the mosaics and EXIF numbers of every scene (tests/raw_ref.py rebuilds the files from them) and
the reference's outputs.  Seeds are walked until no post-processing input puts rgb_lin / exposure within 1e-9 of the
sRGB branch point 0.0031308 and no unclipped srgb * 255 lies within 1e-6 of an integer, so that neither a branch nor an
8-bit truncation can flip for rounding reasons; both conditions are asserted.
"""

import enum
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import make_golden as G  # noqa: E402

OUT = os.path.join(HERE, 'raw_utils.npz')
DEMOSAIC_SIZES = ((2, 2), (2, 6), (4, 2), (6, 10), (34, 66))
COLOR_MATRIX = (0.9, -0.3, -0.1, -0.4, 1.2, 0.2, -0.05, 0.2, 0.6)
NEUTRAL = (0.55, 1.0, 0.62)
NOISE = (2e-4, 1e-6)


class DataSplit(enum.Enum):
  TRAIN = 'train'
  TEST = 'test'


def install():
  jax = G.install_jax_standin()
  jnp = jax.numpy
  to32 = lambda x: np.asarray(x, np.float32) if isinstance(x, np.ndarray) and x.dtype == np.float64 else x
  jnp.array = lambda x, dtype=None: np.array(to32(np.asarray(x)), dtype=dtype)
  jax.jit = lambda fn: (lambda *a: fn(*[to32(v) for v in a]))
  rawpy = types.ModuleType('rawpy')
  rawpy.imread = lambda f: types.SimpleNamespace(raw_image=np.load(f))
  sys.modules['rawpy'] = rawpy
  utils_stub = types.ModuleType('internal.utils')
  utils_stub.file_exists = os.path.exists
  utils_stub.open_file = open
  utils_stub.DataSplit = DataSplit
  sys.modules['internal.utils'] = utils_stub
  sys.path.insert(0, G.REF)
  from internal import raw_utils
  return raw_utils


def fmt(values):
  return ' '.join(repr(float(v)) for v in values)


def make_exif(shutter_den, black=64, white=1023, strings=False):
  return dict(BlackLevel=str(black) if strings else black, WhiteLevel=str(white) if strings else white,
              AsShotNeutral=fmt(NEUTRAL), ColorMatrix2=fmt(COLOR_MATRIX), NoiseProfile=fmt(NOISE), ShutterSpeed=f'1/{shutter_den}')


def write_image(directory, name, mosaic, exif):
  os.makedirs(directory, exist_ok=True)
  with open(os.path.join(directory, name + '.dng'), 'wb') as f:
    np.save(f, mosaic)
  with open(os.path.join(directory, name + '.json'), 'w') as f:
    json.dump([exif], f)


def record_dataset(g, tag, images, meta, testscene):
  g[f'{tag}/images'] = np.asarray(images)
  assert g[f'{tag}/images'].dtype == np.float32
  g[f'{tag}/exposure'] = np.float64(meta['exposure'])
  g[f'{tag}/exposure_levels'] = np.array([meta['exposure_levels'][p] for p in (80, 90, 97, 99, 100)], np.float64)
  g[f'{tag}/exposure_idx'] = np.asarray(meta['exposure_idx'])
  g[f'{tag}/exposure_values'] = np.asarray(meta['exposure_values'], np.float64)
  g[f'{tag}/unique_shutters'] = np.asarray(meta['unique_shutters'], np.float64)
  g[f'{tag}/cam2rgb'] = np.asarray(meta['cam2rgb'], np.float64)
  g[f'{tag}/testscene'] = np.array(bool(testscene))


def main():
  raw_utils = install()
  g = {}
  rs = np.random.default_rng(20240611)

  # bilinear_demosaic, float32
  for h, w in DEMOSAIC_SIZES:
    mosaic = rs.integers(0, 1024, (h, w)).astype(np.uint16)
    out = raw_utils.bilinear_demosaic(mosaic.astype(np.float32), xnp=np)
    assert out.dtype == np.float32 and out.shape == (h, w, 3)
    g[f'demosaic/{h}x{w}/mosaic'] = mosaic
    g[f'demosaic/{h}x{w}/rgb'] = out

  # process_exif on numeric and on string-valued levels
  dens = (30, 60, 120, 60, 30)
  for tag, strings in (('numeric', False), ('strings', True)):
    exifs = [make_exif(d, black=64 + i, white=1023 - i, strings=strings) for i, d in enumerate(dens)]
    meta = raw_utils.process_exif(exifs)
    for k, v in meta.items():
      g[f'exif/{tag}/{k}'] = np.asarray(v, np.float64)
  g['exif/shutter_den'] = np.array(dens)
  g['exif/color_matrix'], g['exif/neutral'], g['exif/noise'] = np.array(COLOR_MATRIX), np.array(NEUTRAL), np.array(NOISE)

  # load_raw_dataset: a plain scene, and a test scene with hdrplus_test/merged
  with tempfile.TemporaryDirectory() as tmp:
    plain = os.path.join(tmp, 'plain')
    names = [f'img{i:02d}.jpg' for i in range(5)]
    mosaics = rs.integers(40, 1024, (5, 12, 16)).astype(np.uint16)
    black, white = np.array([64, 63, 65, 64, 62]), np.array([1023, 1020, 1023, 1000, 1023])
    for i, n in enumerate(names):
      write_image(os.path.join(plain, 'raw'), n[:-4], mosaics[i], make_exif(dens[i], int(black[i]), int(white[i])))
    g['plain/mosaics'], g['plain/black'], g['plain/white'], g['plain/shutter_den'] = mosaics, black, white, np.array(dens)
    for n_down in (1, 2):
      images, meta, testscene = raw_utils.load_raw_dataset(DataSplit.TRAIN, plain, names, 97., n_down)
      record_dataset(g, f'plain/n{n_down}', images, meta, testscene)

    scene = os.path.join(tmp, 'testscene')
    train_m = rs.integers(40, 1024, (4, 12, 16)).astype(np.uint16)
    test_m = rs.integers(40, 1024, (3, 12, 16)).astype(np.uint16)
    merged = rs.integers(4 * 40, 4 * 1024, (12, 16)).astype(np.uint16)
    train_den, test_den = (30, 120, 60, 30), (240, 60, 15)
    colmap_names = ['first.jpg'] + [f't{i}.jpg' for i in range(4)]              # the first one is the test image's copy
    for i in range(4):
      write_image(os.path.join(scene, 'raw', 'train'), f't{i}', train_m[i], make_exif(train_den[i]))
    for i in range(3):
      write_image(os.path.join(scene, 'raw', 'test'), f'x{i}', test_m[i], make_exif(test_den[i]))
    os.makedirs(os.path.join(scene, 'hdrplus_test'))
    with open(os.path.join(scene, 'hdrplus_test', 'merged.dng'), 'wb') as f:
      np.save(f, merged)
    g['testscene/train_mosaics'], g['testscene/test_mosaics'], g['testscene/merged'] = train_m, test_m, merged
    g['testscene/train_den'], g['testscene/test_den'] = np.array(train_den), np.array(test_den)
    for split in (DataSplit.TRAIN, DataSplit.TEST):
      images, meta, testscene = raw_utils.load_raw_dataset(split, scene, colmap_names, 97., 1)
      assert testscene
      record_dataset(g, f'testscene/{split.value}', images, meta, testscene)

  # postprocess_raw (float64) and match_images_affine: seeds walked until no branch or truncation is at a rounding edge
  cam2rgb = g['plain/n1/cam2rgb'][0]
  g['post/cam2rgb'] = cam2rgb
  for h, w in ((5, 7), (75, 93)):
    seed = 0
    while True:
      r = np.random.default_rng([seed, h, w])
      raw = (r.uniform(-0.05, 0.6, (h, w, 3)) * r.choice([1., 1., 0.004], (h, w, 1))).astype(np.float32)
      exposure = 0.35
      lin = raw.astype(np.float64) @ cam2rgb.T
      outs = [raw_utils.postprocess_raw(raw.astype(np.float64), cam2rgb, exposure), raw_utils.postprocess_raw(raw.astype(np.float64), cam2rgb)]
      ok = True
      for x, out in zip((exposure, np.percentile(lin, 97)), outs):
        z = lin / x
        ok &= np.abs(z - 0.0031308).min() > 1e-9
        inner = (z > 0) & (z < 1)
        s255 = out[inner] * 255
        ok &= np.abs(s255 - np.rint(s255)).min() > 1e-6
      if ok:
        break
      seed += 1
    z = lin / exposure
    assert (z < 0).any() and (z > 1).any() and ((z > 0) & (z <= 0.0031308)).any() and (z > 0.0031308).any()
    for x, out in zip((exposure, np.percentile(lin, 97)), outs):
      zz = lin / x
      assert np.abs(zz - 0.0031308).min() > 1e-9
      inner = (zz > 0) & (zz < 1)
      assert np.abs(out[inner] * 255 - np.rint(out[inner] * 255)).min() > 1e-6
    g[f'post/{h}x{w}/raw'], g[f'post/{h}x{w}/exposure'], g[f'post/{h}x{w}/seed'] = raw, np.float64(exposure), np.array(seed)
    g[f'post/{h}x{w}/srgb'], g[f'post/{h}x{w}/srgb_auto'] = outs
    g[f'post/{h}x{w}/linear'] = lin
    g[f'post/{h}x{w}/auto_exposure'] = np.float64(np.percentile(lin, 97))

  for h, w in ((3, 4), (75, 93)):
    r = np.random.default_rng([7, h, w])
    gt = r.uniform(0, 1, (h, w, 3)).astype(np.float32)
    est = (gt * np.array([1.3, 0.8, 1.1]) + np.array([0.02, -0.05, 0.1]) + 0.05 * r.normal(size=gt.shape)).astype(np.float32)
    g[f'affine/{h}x{w}/est'], g[f'affine/{h}x{w}/gt'] = est, gt
    g[f'affine/{h}x{w}/matched'] = raw_utils.match_images_affine(est.astype(np.float64), gt.astype(np.float64))
    a, b = raw_utils.best_fit_affine(gt.astype(np.float64), est.astype(np.float64), axis=(0, 1))
    g[f'affine/{h}x{w}/a'], g[f'affine/{h}x{w}/b'] = a, b

  px, py = np.meshgrid(np.arange(7), np.arange(5), indexing='xy')
  g['bayer/pix_x'], g['bayer/pix_y'] = px, py
  g['bayer/mask'] = raw_utils.pixels_to_bayer_mask(px, py)

  np.savez_compressed(OUT, **g)
  print(f'wrote {OUT}: {len(g)} arrays, {os.path.getsize(OUT)} bytes')
  assert os.path.getsize(OUT) < 1000000


if __name__ == '__main__':
  main()
