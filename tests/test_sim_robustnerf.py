"""tests/test_gpu_robustnerf.py's kernel-level part, run on the kernel-source simulator in a child pytest
(MNR_TESTS_ON_SIMULATOR=1, the way tests/test_sim_gpu_suite.py runs the other `-m gpu` files): mnr_robustnerf_mask and
mnr_quantile against the reference's recorded outputs and NumPy, and the argument errors, with the test code unchanged.
The composed cases need the MI355X run (or MNR_TESTS_ON_SIMULATOR=1 by hand: a few minutes of simulator time)."""

import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(not (shutil.which('clang++') or os.path.exists('/opt/rocm/lib/llvm/bin/clang++')),
                                reason='needs clang++')


def test_robustnerf_kernels_pass_on_the_simulator():
  env = dict(os.environ, MNR_TESTS_ON_SIMULATOR='1')
  cmd = [sys.executable, '-m', 'pytest', '-q', '-m', 'gpu', '-p', 'no:cacheprovider', 'tests/test_gpu_robustnerf.py', '-k',
         'mask_kernel or quantile or argument_errors']
  r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
  tail = '\n'.join((r.stdout + r.stderr).splitlines()[-25:])
  assert r.returncode == 0, tail
  assert ' passed' in tail and 'failed' not in tail and 'skipped' not in tail, tail
