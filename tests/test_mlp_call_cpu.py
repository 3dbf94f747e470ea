"""MLP.__call__ on caller-supplied Gaussians, without a GPU: the two C entries are declared and bound, the source file is on
every build list, an MLP that belongs to no built model refuses the call, and the documents describe the callable."""

import os

import pytest
import torch

from multinerf_amd import _lib, build, models
from tests.sim_helpers import tool_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('mnr_ipe_from_gaussians', 'mnr_ipe_from_gaussians_tangent')


def test_header_declares_and_protos_bind_both_entries():
  names = _lib.header_symbols()
  for e in ENTRIES:
    assert e in names and e in _lib._PROTOS and e not in _lib.F32_ABSENT
  # (cfg, M, means, covs, basis, feat_out, ld_feat, feat_f32_out, means_out, covs_out, stream) / (..., feat_out, ld_feat, stream)
  assert len(_lib._PROTOS[ENTRIES[0]][0]) == 11 and len(_lib._PROTOS[ENTRIES[1]][0]) == 8
  with open(_lib.HEADER_PATH) as f:
    text = f.read()
  assert 'models.py:403-409' in text                      # the reference lines the entries replace


def test_source_file_is_on_every_build_list():
  assert 'gaussians.hip' in build.SOURCES and 'gaussians.hip' in build.SOURCES_F32
  for rel, attr in (('hipsim/build.py', 'SOURCES'), ('isa_report.py', 'KERNEL_FILES')):
    assert 'gaussians.hip' in getattr(tool_module(rel), attr), rel
  with open(os.path.join(build.CSRC, 'gaussians.hip')) as f:
    src = f.read()
  assert '#pragma clang fp contract(off)' in src and '#include "ipe_math.h"' in src


def test_encode_body_is_shared_not_copied():
  """csrc/ipe_encode_body.inc is the one encode loop / write-out of both featurisation kernels, and is on the lists that
  decide whether a built library is stale."""
  inc = 'ipe_encode_body.inc'
  assert os.path.join(build.CSRC, inc) in build.HEADERS
  assert os.path.join(build.CSRC, inc) in tool_module('hipsim/build.py').DEPS
  srcs = {}
  for name in sorted(os.listdir(build.CSRC)):
    with open(os.path.join(build.CSRC, name)) as f:
      srcs[name] = f.read()
  for name in ('features.hip', 'gaussians.hip'):
    assert '#include "%s"' % inc in srcs[name], name
  for gone in ('fe_sincos_wrapped', 'GsTangent', 'GS_THREADS'):
    assert gone not in srcs['gaussians.hip'], gone
  assert sum(text.count('struct FeTangent') for text in srcs.values()) == 1


def test_mlp_of_an_unbuilt_model_raises():
  model = models.Model()
  g = (torch.zeros((1, 4, 3)), torch.zeros((1, 4, 3, 3)))
  for mlp in (model.nerf_hp, model.prop_hp, models.NerfMLP()):
    with pytest.raises(RuntimeError, match='not attached'):
      mlp(None, g, viewdirs=torch.zeros((1, 3)))


def test_points_to_gaussians():
  xyz = torch.arange(12, dtype=torch.float32).reshape(2, 2, 3)
  means, covs = models.points_to_gaussians(xyz, 0.5)
  assert torch.equal(means, xyz) and covs.shape == (2, 2, 3, 3)
  assert torch.equal(covs, (0.25 * torch.eye(3)).expand(2, 2, 3, 3))
  assert (models.points_to_gaussians(xyz)[1] == 0).all()


def test_documents_describe_the_callable():
  with open(os.path.join(ROOT, 'README.md')) as f:
    readme = f.read()
  assert 'not callable' not in readme and 'model.nerf_hp(' in readme and 'query_density' in readme
  with open(os.path.join(ROOT, 'INTEGRATION.md')) as f:
    assert 'mnr_ipe_from_gaussians' in f.read()
