"""Synthetic scenes on disk for the dataset tests (tests/test_datasets_tat_cpu.py, tests/test_gpu_ingest.py): Tanks and Temples
in the NeRF++ and the Free View Synthesis layouts, Blender PNG / TIFF scenes and an NGP-style LLFF scene, written from
cameras and pixels the caller chose."""

import json
import os

import numpy as np

FLIP = np.diag([1., -1., -1., 1.])


def ring_cameras(n, radius=1.5, seed=0):
  """[n,4,4] camera-to-world matrices in this code's frame (x right, y up, z back): cameras on a wobbly ring, looking at the origin."""
  rs = np.random.default_rng(seed)
  out = []
  for i in range(n):
    phi = 2 * np.pi * i / n + 0.1 * rs.normal()
    c = radius * np.array([np.cos(phi), np.sin(phi), 0.3 + 0.2 * rs.normal()])
    back = c / np.linalg.norm(c)
    right = np.cross([0., 0., 1.], back)
    right /= np.linalg.norm(right)
    up = np.cross(back, right)
    m = np.eye(4)
    m[:3, :4] = np.stack([right, up, back, c], -1)
    out.append(m)
  return np.stack(out, 0)


def random_images(n, h, w, c=3, seed=0):
  return np.random.default_rng([seed, n, h, w, c]).integers(0, 256, (n, h, w, c), dtype=np.uint8)


def write_nerfpp_split(root, split, names, c2w, focal, images=None):
  """`<root>/<split>/{pose,intrinsics,rgb}/<name>.{txt,txt,png}`; the files are written in the order of `names` (any order),
  c2w [n,4,4] are the cameras in THIS code's frame (the files hold them in the NeRF++ frame: times diag(1,-1,-1,1))."""
  from PIL import Image
  for d in ('pose', 'intrinsics', 'rgb'):
    os.makedirs(os.path.join(root, split, d), exist_ok=True)
  for i, name in enumerate(names):
    np.savetxt(os.path.join(root, split, 'pose', name + '.txt'), (c2w[i] @ FLIP).reshape(1, 16), fmt='%.17g')
    h, w = (images.shape[1:3] if images is not None else (2 * focal, 2 * focal))
    K = np.array([[focal + i, 0, w / 2., 0], [0, focal + i, h / 2., 0], [0, 0, 1, 0], [0, 0, 0, 1.]])   # (only the first is used)
    np.savetxt(os.path.join(root, split, 'intrinsics', name + '.txt'), K.reshape(1, 16), fmt='%.17g')
    if images is not None:
      Image.fromarray(images[i]).save(os.path.join(root, split, 'rgb', name + '.png'))


def write_fvs_size(root, dirname, c2w, focal, images):
  """`<root>/dense/<dirname>/{im_%08d.png, Ks.npy, Rs.npy, ts.npy}` with COLMAP world-to-camera matrices of the cameras c2w."""
  from PIL import Image
  d = os.path.join(root, 'dense', dirname)
  os.makedirs(d, exist_ok=True)
  w2c = np.linalg.inv(c2w @ FLIP)
  np.save(os.path.join(d, 'Rs.npy'), w2c[:, :3, :3])
  np.save(os.path.join(d, 'ts.npy'), w2c[:, :3, 3])
  h, w = images.shape[1:3]
  np.save(os.path.join(d, 'Ks.npy'), np.stack([np.array([[focal + i, 0, w / 2.], [0, focal + i, h / 2.], [0, 0, 1.]]) for i in range(len(c2w))]))
  for i in reversed(range(len(c2w))):
    Image.fromarray(images[i]).save(os.path.join(d, f'im_{i:08d}.png'))
  with open(os.path.join(d, 'notes.txt'), 'w') as f:       # (a file that is no image)
    f.write('x')


def write_blender_scene(root, n=4, size=12, seed=0, tiffs=False, disps=False):
  """transforms_{train,test}.json with r_<i>.png (RGBA) and r_<i>_normal.png (RGB); tiffs: r_<i>_{R,G,B,A}.tiff, disps:
  r_<i>_disp.tiff (float32, single channel).  Returns {split: dict of the arrays written}."""
  from PIL import Image
  rs = np.random.default_rng(seed)
  wrote = {}
  for split in ('train', 'test'):
    frames = []
    os.makedirs(os.path.join(root, split), exist_ok=True)
    rgba = rs.integers(0, 256, (n, size, size, 4), dtype=np.uint8)
    rgba[:, 0, :3, 3], rgba[:, 1, :3, 3] = 0, 255
    nrm = rs.integers(0, 256, (n, size, size, 3), dtype=np.uint8)
    lin = rs.uniform(0, 1, (n, size, size, 4)).astype(np.float32)
    lin[:, :5, :5] = 0.001                                   # (a block below the end of the sRGB curve's linear segment)
    disp = rs.uniform(0.1, 2, (n, size, size)).astype(np.float32)
    for i in range(n):
      prefix = os.path.join(root, split, f'r_{i}')
      Image.fromarray(rgba[i], 'RGBA').save(prefix + '.png')
      Image.fromarray(nrm[i], 'RGB').save(prefix + '_normal.png')
      if tiffs:
        for k, ch in enumerate('RGBA'):
          Image.fromarray(lin[i, ..., k]).save(prefix + f'_{ch}.tiff')
      if disps:
        Image.fromarray(disp[i]).save(prefix + '_disp.tiff')
      m = np.eye(4)
      m[:3, 3] = [0.1 * i, 0.2, 4.0]
      frames.append({'file_path': f'./{split}/r_{i}', 'transform_matrix': m.tolist()})
    with open(os.path.join(root, f'transforms_{split}.json'), 'w') as f:
      json.dump({'camera_angle_x': 0.7, 'frames': frames}, f)
    wrote[split] = dict(rgba=rgba, normals=nrm, linear=lin, disp=disp)
  return wrote


def write_llff_scene(root, n=8, size=(6, 8), seed=2):
  """An NGP-style scene: transforms.json and images/<i>.png (RGB).  Returns the pixels [n,h,w,3]."""
  from PIL import Image
  os.makedirs(os.path.join(root, 'images'))
  rs = np.random.default_rng(seed)
  h, w = size
  pixels = rs.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
  frames = []
  for i in range(n):
    Image.fromarray(pixels[i]).save(os.path.join(root, 'images', f'{i}.png'))
    m = np.eye(4)
    m[:3, :3] += 0.05 * rs.normal(size=(3, 3))
    m[:3, 3] = rs.normal(size=3) * 0.3
    frames.append({'file_path': f'images/{i}.png', 'transform_matrix': m.tolist()})
  with open(os.path.join(root, 'transforms.json'), 'w') as f:
    json.dump({'w': w, 'h': h, 'fl_x': 10.0, 'fl_y': 10.0, 'frames': frames}, f)
  return pixels
