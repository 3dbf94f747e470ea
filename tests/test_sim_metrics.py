"""tests/test_gpu_metrics.py's kernel-level part, run on the kernel-source simulator in a child pytest
(MNR_TESTS_ON_SIMULATOR=1, the way tests/test_sim_robustnerf.py runs its file): mnr_ssim, mnr_image_sqdiff, mnr_cc_gram and
mnr_cc_apply against the reference's recorded outputs and the float64 restatements, image.color_correct and MetricHarness
on top of them, and the argument errors, with the test code unchanged.  evaluate_image's composed case runs there too (it
needs no model); the train.py / eval.py case needs the MI355X."""

import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(not (shutil.which('clang++') or os.path.exists('/opt/rocm/lib/llvm/bin/clang++')),
                                reason='needs clang++')


def test_metric_kernels_pass_on_the_simulator():
  env = dict(os.environ, MNR_TESTS_ON_SIMULATOR='1')
  cmd = [sys.executable, '-m', 'pytest', '-q', '-m', 'gpu', '-p', 'no:cacheprovider', 'tests/test_gpu_metrics.py', '-k',
         'kernel or color_correct or metric_harness or argument_errors or evaluate_image']
  r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
  tail = '\n'.join((r.stdout + r.stderr).splitlines()[-25:])
  assert r.returncode == 0, tail
  assert ' passed' in tail and 'failed' not in tail and 'skipped' not in tail, tail
