"""tests/test_gpu_mesh.py run on the kernel-source simulator in a child pytest (MNR_TESTS_ON_SIMULATOR=1, the way
tests/test_sim_ingest.py runs its file): the three kernels of csrc/mesh.hip (classification, the ballot / popcount prefix
across waves and workgroups, vertex and face emission) against the NumPy restatement on every field and shape of that file,
determinism, the degenerate fields and density_grid on the analytic sphere, with the test code unchanged.  The model and the
script are left to the MI355X: they run no kernel of this file's subject that the other tests do not."""

import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(not (shutil.which('clang++') or os.path.exists('/opt/rocm/lib/llvm/bin/clang++')),
                                reason='needs clang++')


def test_mesh_kernels_pass_on_the_simulator():
  env = dict(os.environ, MNR_TESTS_ON_SIMULATOR='1')
  cmd = [sys.executable, '-m', 'pytest', '-q', '-m', 'gpu', '-p', 'no:cacheprovider', 'tests/test_gpu_mesh.py', '-k', 'not script and not model']
  r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
  tail = '\n'.join((r.stdout + r.stderr).splitlines()[-25:])
  assert r.returncode == 0, tail
  assert ' passed' in tail and 'failed' not in tail and 'skipped' not in tail, tail


def test_emit_passes_tolerate_a_stale_workspace():
  """include/mnerf.h: with a mask and offsets that are not this field's, the emit passes ignore mask bits of edges that leave
  the grid and write nothing at or beyond row n_verts / n_faces.  Run on the simulator build with host buffers and canaries."""
  import ctypes as C

  import torch

  from multinerf_amd import _lib as L
  from tests import sim_helpers as S
  lib = S.load_sim()
  lib.hipsim_reset(0, 0)
  nx, ny, nz = 3, 4, 5
  n = nx * ny * nz
  field = torch.linspace(-1., 1., n).reshape(nx, ny, nz).contiguous()
  mask = torch.full((n,), 0x7f, dtype=torch.uint8)                      # every edge "carries a vertex", also those leaving the grid
  offsets = torch.zeros((1, 2), dtype=torch.int64)
  base = torch.full((n,), -7, dtype=torch.int32)
  V, T, pad = 10, 6, 64
  verts, normals = torch.full((V + pad, 3), 9., dtype=torch.float32), torch.full((V + pad, 3), 9., dtype=torch.float32)
  faces = torch.full((T + pad, 3), -9, dtype=torch.int32)
  a = L.MtArgs()
  a.nx, a.ny, a.nz, a.field, a.level, a.spacing = nx, ny, nz, field.data_ptr(), 0., 1.
  a.mask, a.offsets, a.base = mask.data_ptr(), offsets.data_ptr(), base.data_ptr()
  a.verts, a.normals, a.n_verts, a.faces, a.n_faces = verts.data_ptr(), normals.data_ptr(), V, faces.data_ptr(), T
  assert lib.mnr_mt_workgroups(n) == 1
  S.sim_check(lib, lib.mnr_mt_emit_vertices(C.byref(a), None))
  S.sim_check(lib, lib.mnr_mt_emit_faces(C.byref(a), None))
  assert (verts[V:] == 9.).all() and (normals[V:] == 9.).all() and (faces[T:] == -9).all()
  assert torch.isfinite(verts[:V]).all() and (verts[:V] >= 0).all() and (verts[:V] <= torch.tensor([nx - 1., ny - 1., nz - 1.])).all()
  # the base ids count in-grid edges only: point 0 has all 7, the last point none
  assert base[0] == 0 and base[1] == 7 and base[n - 1] == base[n - 2] + 1
