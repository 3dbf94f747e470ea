"""tests/test_gpu_raw.py's kernel-level, dataset and evaluate_image parts, run on the kernel-source simulator in a child pytest
(MNR_TESTS_ON_SIMULATOR=1, the way tests/test_sim_render.py runs its file): mnr_raw_demosaic, mnr_raw_postprocess,
mnr_quantile_f64, mnr_affine_sums / mnr_affine_apply against the reference's recorded outputs, the argument errors, the raw
LLFF scenes on disk and the procedural raw capture, with the test code unchanged.  The 100003-value percentile is included:
it is the one case whose radix select runs on several workgroups (merged histograms, per-workgroup minima, the grid-stride
tail).  Only the scripts (tests/test_gpu_raw_scripts.py) need the MI355X."""

import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(not (shutil.which('clang++') or os.path.exists('/opt/rocm/lib/llvm/bin/clang++')),
                                reason='needs clang++')


def test_raw_kernels_pass_on_the_simulator():
  env = dict(os.environ, MNR_TESTS_ON_SIMULATOR='1')
  cmd = [sys.executable, '-m', 'pytest', '-q', '-m', 'gpu', '-p', 'no:cacheprovider', 'tests/test_gpu_raw.py']
  r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
  tail = '\n'.join((r.stdout + r.stderr).splitlines()[-25:])
  assert r.returncode == 0, tail
  assert ' passed' in tail and 'failed' not in tail and 'skipped' not in tail, tail
