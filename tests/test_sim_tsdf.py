"""tests/test_gpu_tsdf.py run on the kernel-source simulator in a child pytest (MNR_TESTS_ON_SIMULATOR=1, the way
tests/test_sim_mesh.py runs its file): both kernels of csrc/tsdf.hip (the brick mapping with its ragged bricks, the staging of
the matrices, the per-brick culling and its ballot compaction, the launches of a stack longer than one
launch stages, vertex validity) against the NumPy restatement bit for bit, with the test code unchanged.  The model and the
script are left to the MI355X: they run no kernel of this file's subject that the other tests do not."""

import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(not (shutil.which('clang++') or os.path.exists('/opt/rocm/lib/llvm/bin/clang++')),
                                reason='needs clang++')


def test_tsdf_kernels_pass_on_the_simulator():
  env = dict(os.environ, MNR_TESTS_ON_SIMULATOR='1')
  cmd = [sys.executable, '-m', 'pytest', '-q', '-m', 'gpu', '-p', 'no:cacheprovider', 'tests/test_gpu_tsdf.py', '-k',
         'not script and not renders']
  r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
  tail = '\n'.join((r.stdout + r.stderr).splitlines()[-25:])
  assert r.returncode == 0, tail
  assert ' passed' in tail and 'failed' not in tail and 'skipped' not in tail, tail
