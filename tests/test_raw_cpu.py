"""The host side of the RawNeRF data path (no GPU): EXIF processing against the reference's recorded output, the raw file
loader's pairing and errors, the synthetic capture, the C ABI's new symbols, and what configs and docs say."""

import ctypes
import dataclasses
import json
import os
import re

import numpy as np
import pytest

from multinerf_amd import _lib as L
from multinerf_amd import configs, raw_utils
from tests import raw_ref as ref
from tests.sim_helpers import tool_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('mnr_raw_demosaic', 'mnr_raw_postprocess', 'mnr_quantile_f64_workspace', 'mnr_quantile_f64',
               'mnr_affine_sums_partials', 'mnr_affine_sums', 'mnr_affine_apply')


@pytest.fixture(scope='module')
def g():
  return np.load(os.path.join(ROOT, 'tests', 'golden', 'raw_utils.npz'))


@pytest.mark.parametrize('tag,strings', [('numeric', False), ('strings', True)])
def test_process_exif_equals_the_reference(g, tag, strings):
  exifs = [ref.make_exif(g, d, 64 + i, 1023 - i, strings=strings) for i, d in enumerate(g['exif/shutter_den'])]
  meta = raw_utils.process_exif(exifs)
  keys = [k[len(f'exif/{tag}/'):] for k in g.files if k.startswith(f'exif/{tag}/')]
  assert sorted(meta) == sorted(keys)
  for k in keys:
    want = g[f'exif/{tag}/{k}']
    assert np.asarray(meta[k]).shape == want.shape, k
    assert np.abs(np.asarray(meta[k], np.float64) - want).max() <= 1e-12, k
  assert meta['cam2rgb'].shape == (5, 3, 3) and meta['ShutterSpeed'][2] == 1 / 120
  with pytest.raises(ValueError, match='neither a number nor a string'):
    raw_utils.process_exif([dict(exifs[0], BlackLevel=[64, 64])])


def test_load_raw_images_pairs_npy_with_json_and_reports_what_is_missing(g, tmp_path):
  d = str(tmp_path / 'raw')
  with pytest.raises(ValueError, match='does not exist'):
    raw_utils.load_raw_images(d)
  names = ['b.jpg', 'a.png', 'c']
  for i, n in enumerate(names):
    ref.write_image(d, os.path.splitext(n)[0], g['plain/mosaics'][i], ref.make_exif(g, (30, 60, 120)[i]))
  raws, exifs = raw_utils.load_raw_images(d, names)                                   # extensions are ignored, order is kept
  assert raws.dtype == np.uint16 and np.array_equal(raws, g['plain/mosaics'][:3])
  assert [e['ShutterSpeed'] for e in exifs] == ['1/30', '1/60', '1/120']
  raws_all, exifs_all = raw_utils.load_raw_images(d)                                  # every mosaic of the folder, sorted
  assert np.array_equal(raws_all, g['plain/mosaics'][[1, 0, 2]]) and exifs_all[0]['ShutterSpeed'] == '1/60'
  with pytest.raises(ValueError) as e:
    raw_utils.load_raw_images(d, ['missing.jpg'])
  assert 'missing.dng' in str(e.value) and 'missing.npy' in str(e.value) and 'rawpy' in str(e.value)
  os.remove(os.path.join(d, 'c.json'))
  with pytest.raises(ValueError, match=r'c\.json'):
    raw_utils.load_raw_images(d, ['c'])
  np.save(os.path.join(d, 'f.npy'), np.zeros((4, 4), np.float32))
  with pytest.raises(ValueError, match='2-D uint16'):
    raw_utils.load_raw_images(d, ['f'])
  empty = str(tmp_path / 'empty')
  os.makedirs(empty)
  with pytest.raises(ValueError, match='No raw images'):
    raw_utils.load_raw_images(empty)


def test_synthesize_raw_capture_is_deterministic_and_in_exiftool_form():
  rs = np.random.default_rng(3)
  images = rs.uniform(0, 1, (4, 6, 8, 3))
  m1, e1 = raw_utils.synthesize_raw_capture(images, 'train', seed=0)
  m2, e2 = raw_utils.synthesize_raw_capture(images, 'train', seed=0)
  m3, _ = raw_utils.synthesize_raw_capture(images, 'train', seed=1)
  mt, et = raw_utils.synthesize_raw_capture(images, 'test', seed=0)
  assert m1.dtype == np.uint16 and m1.shape == (4, 6, 8) and np.array_equal(m1, m2) and e1 == e2
  assert not np.array_equal(m1, m3) and not np.array_equal(m1, mt)
  assert m1.min() >= 0 and m1.max() <= 1023
  assert [e['ShutterSpeed'] for e in e1] == ['1/30', '1/60', '1/120', '1/30'] and {e['ShutterSpeed'] for e in et} == {'1/30'}
  assert isinstance(e1[0]['BlackLevel'], int) and e1[0]['BlackLevel'] == 64 and e1[0]['WhiteLevel'] == 1023
  for k in ('AsShotNeutral', 'ColorMatrix2', 'NoiseProfile'):
    assert isinstance(e1[0][k], str) and all(float(v) == float(v) for v in e1[0][k].split(' '))
  json.dumps([e1[0]])
  # the clean signal: 0.25 x the image through the RGGB pattern, scaled by the relative shutter, within the noise
  want = 64 + 959 * 0.25 * images[0, 0, 0, 0]
  assert abs(float(m1[0, 0, 0]) - want) <= 959 * 6 * np.sqrt(1e-4 * 0.25 + 1e-6) + 0.5
  meta = raw_utils.process_exif(e1)
  assert np.allclose(meta['cam2rgb'][0], np.eye(3), atol=1e-6)
  with pytest.raises(ValueError, match='even height and width'):
    raw_utils.synthesize_raw_capture(images[:, :5], 'train')


def test_header_bindings_and_both_libraries_agree_on_the_new_symbols():
  missing = [os.path.basename(p) for p in (L.LIB_PATH, L.LIB_F32_PATH) if not os.path.exists(p)]
  if missing:
    pytest.skip(f'{", ".join(missing)} not built')
  declared = L.header_symbols()
  for name in NEW_SYMBOLS:
    assert name in declared and name in L._PROTOS, name
  assert set(L._PROTOS) <= set(declared)
  from multinerf_amd import build
  assert 'raw.hip' in build.SOURCES and 'raw.hip' in build.SOURCES_F32
  for path in (L.LIB_PATH, L.LIB_F32_PATH):
    lib = ctypes.CDLL(path)
    for name in NEW_SYMBOLS:
      assert hasattr(lib, name), (path, name)
    lib.mnr_abi_version.restype = ctypes.c_int
    assert lib.mnr_abi_version() == 21
  with open(L.HEADER_PATH) as f:
    header = f.read()
  assert re.search(r'MNR_RAW_U16 = 0, MNR_RAW_F32 = 1', header) and L.RAW_DTYPE == {'uint16': 0, 'float32': 1}
  assert ctypes.sizeof(L.RawPostArgs) == 8 + 8 + 8 + 72 + 8 + 8 + 8 + 8 + 8 + 8


def test_simulator_and_tools_list_the_new_kernel_file():
  for rel, attr in (('hipsim/build.py', 'SOURCES'), ('isa_report.py', 'KERNEL_FILES')):
    assert 'raw.hip' in getattr(tool_module(rel), attr), rel
  digests = json.load(open(os.path.join(ROOT, 'profiles', 'r6_validated_isa.json')))['kernels']
  for kernel in ('raw_demosaic_quad_kernel', 'raw_demosaic_down_kernel', 'raw_postprocess_kernel', 'quantile_f64_hist_kernel',
                 'quantile_f64_above_kernel', 'quantile_f64_final_kernel', 'affine_sums_kernel', 'affine_apply_kernel'):
    assert any(kernel in n for n in digests), kernel


def test_configs_and_docs_no_longer_claim_the_refusal():
  cfg = configs.load_preset('llff_raw', [])
  assert cfg.rawnerf_mode and cfg.apply_bayer_mask and cfg.data_loss_type == 'rawnerf'
  assert dataclasses.replace(cfg, eval_raw_affine_cc=True).eval_raw_affine_cc
  read = lambda rel: open(os.path.join(ROOT, rel)).read()
  assert 'RawNeRF post-processing is not supported' not in read('README.md')
  assert 'raw_utils' in read('README.md') and '.npy' in read('README.md') and 'rawpy' in read('README.md')
  for rel in ('multinerf_amd/datasets.py', 'render.py', 'eval.py'):
    text = read(rel)
    assert 'RawNeRF inputs need rawpy' not in text and 'rawnerf_mode is not supported' not in text, rel
  assert 'raw.hip' in read('DESIGN.md') and 'mnr_raw_demosaic' in read('INTEGRATION.md')
