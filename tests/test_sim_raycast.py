"""tests/test_gpu_raycast.py run on the kernel-source simulator in a child pytest (MNR_TESTS_ON_SIMULATOR=1, the way
tests/test_sim_shtex.py runs its file): the two kernels of csrc/meshray.hip through the product's own host code against the NumPy
restatement bit for bit, the independence of grid and ray order, watertightness, the analytic sphere through every camera model,
the rasteriser agreement and the argument checks, with the test code unchanged.  The script is left to the MI355X."""

import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(not (shutil.which('clang++') or os.path.exists('/opt/rocm/lib/llvm/bin/clang++')),
                                reason='needs clang++')


def test_raycast_kernels_pass_on_the_simulator():
  env = dict(os.environ, MNR_TESTS_ON_SIMULATOR='1')
  cmd = [sys.executable, '-m', 'pytest', '-q', '-m', 'gpu', '-p', 'no:cacheprovider', 'tests/test_gpu_raycast.py', '-k', 'not script']
  r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
  tail = '\n'.join((r.stdout + r.stderr).splitlines()[-25:])
  assert r.returncode == 0, tail
  assert ' passed' in tail and 'failed' not in tail and 'skipped' not in tail, tail
