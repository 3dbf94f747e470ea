"""tests/test_gpu_registration.py run on the kernel-source simulator in a child pytest (MNR_TESTS_ON_SIMULATOR=1, the way
tests/test_sim_geometry.py runs its file): the kernels of csrc/meshreg.hip through the product's own host code against the NumPy
restatement: closest points and normals bit for bit, the sums, the crop volume, the registration against the float64 ICP, the
metrics and the argument checks, with the test code unchanged.  The script is left to the MI355X: its child process would load the
device build."""

import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(not (shutil.which('clang++') or os.path.exists('/opt/rocm/lib/llvm/bin/clang++')),
                                reason='needs clang++')


def test_registration_kernels_pass_on_the_simulator():
  env = dict(os.environ, MNR_TESTS_ON_SIMULATOR='1')
  cmd = [sys.executable, '-m', 'pytest', '-q', '-m', 'gpu', '-p', 'no:cacheprovider', 'tests/test_gpu_registration.py', '-k', 'not script']
  r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
  tail = '\n'.join((r.stdout + r.stderr).splitlines()[-25:])
  assert r.returncode == 0, tail
  assert ' passed' in tail and 'failed' not in tail and 'skipped' not in tail, tail
