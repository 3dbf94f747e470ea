"""Host helpers of the RawNeRF tests: float64 NumPy restatements (independent of the product code) and the writers that
rebuild the golden scenes of tests/golden/raw_utils.npz on disk in the documented `.npy` + `.json` layout."""

import json
import os

import numpy as np

_F32_EPS = float(np.finfo(np.float32).eps)


def fmt(values):
  return ' '.join(repr(float(v)) for v in values)


def make_exif(g, shutter_den, black=64, white=1023, strings=False):
  """The EXIF dict tests/golden/make_golden_raw.py wrote for one image (exiftool's form)."""
  return dict(BlackLevel=str(int(black)) if strings else int(black), WhiteLevel=str(int(white)) if strings else int(white),
              AsShotNeutral=fmt(g['exif/neutral']), ColorMatrix2=fmt(g['exif/color_matrix']), NoiseProfile=fmt(g['exif/noise']),
              ShutterSpeed=f'1/{int(shutter_den)}')


def write_image(directory, name, mosaic, exif):
  os.makedirs(directory, exist_ok=True)
  np.save(os.path.join(directory, name + '.npy'), np.asarray(mosaic, np.uint16))
  with open(os.path.join(directory, name + '.json'), 'w') as f:
    json.dump([exif], f)


def write_transforms(data_dir, names, rs, w=16, h=12):
  """NGP-style poses for `names` (every file_path must exist: the loader keeps the frames whose file it finds)."""
  frames = []
  os.makedirs(os.path.join(data_dir, 'images'), exist_ok=True)
  for n in names:
    open(os.path.join(data_dir, 'images', n), 'wb').close()
    q, _ = np.linalg.qr(np.eye(3) + 0.1 * rs.normal(size=(3, 3)))
    q = q * np.sign(np.diag(q))
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = q, rs.normal(size=3)
    frames.append(dict(file_path='images/' + n, transform_matrix=m.tolist()))
  with open(os.path.join(data_dir, 'transforms.json'), 'w') as f:
    json.dump(dict(w=w, h=h, fl_x=20., fl_y=20., frames=frames), f)


def write_plain_scene(g, data_dir, rs):
  names = [f'img{i:02d}.jpg' for i in range(5)]
  for i, n in enumerate(names):
    write_image(os.path.join(data_dir, 'raw'), n[:-4], g['plain/mosaics'][i],
                make_exif(g, g['plain/shutter_den'][i], g['plain/black'][i], g['plain/white'][i]))
  write_transforms(data_dir, names, rs)
  return names


def write_test_scene(g, data_dir, rs):
  names = ['first.jpg'] + [f't{i}.jpg' for i in range(4)]
  for i in range(4):
    write_image(os.path.join(data_dir, 'raw', 'train'), f't{i}', g['testscene/train_mosaics'][i], make_exif(g, g['testscene/train_den'][i]))
  for i in range(3):
    write_image(os.path.join(data_dir, 'raw', 'test'), f'x{i}', g['testscene/test_mosaics'][i], make_exif(g, g['testscene/test_den'][i]))
  os.makedirs(os.path.join(data_dir, 'hdrplus_test'), exist_ok=True)
  np.save(os.path.join(data_dir, 'hdrplus_test', 'merged.npy'), g['testscene/merged'])
  write_transforms(data_dir, names, rs)
  return names


def block_mean(img, n):
  """float32(mean over n x n blocks, in float64) of a float32 [H,W,3] image."""
  h, w, c = img.shape
  return img.astype(np.float64).reshape(h // n, n, w // n, n, c).mean((1, 3)).astype(np.float32)


def linear_to_srgb(z):
  return np.where(z <= 0.0031308, 323 / 25 * z, (211 * np.maximum(_F32_EPS, z)**(5 / 12) - 11) / 200)


def postprocess(raw, cam2rgb, exposure):
  lin = np.asarray(raw, np.float64) @ np.asarray(cam2rgb, np.float64).T
  return linear_to_srgb(np.clip(lin / exposure, 0, 1))


def to_u8(img):
  """utils.save_img_u8's quantisation."""
  return (np.clip(np.nan_to_num(img), 0., 1.) * 255.).astype(np.uint8)


def match_affine(est, gt):
  est, gt = np.asarray(est, np.float64), np.asarray(gt, np.float64)
  x_m, y_m = gt.mean((0, 1)), est.mean((0, 1))
  a = ((gt * est).mean((0, 1)) - x_m * y_m) / ((gt * gt).mean((0, 1)) - x_m * x_m)
  b = y_m - a * x_m
  return (est - b) / a
