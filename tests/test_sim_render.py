"""tests/test_gpu_render.py's kernel-level part, run on the kernel-source simulator in a child pytest
(MNR_TESTS_ON_SIMULATOR=1, the way tests/test_sim_metrics.py runs its file): mnr_weighted_percentile, mnr_vis_cmap,
mnr_vis_matte and mnr_spherical_rays against the reference's recorded outputs and the float64 restatements, vis.visualize_cmap
and vis.visualize_suite on top of them, the argument errors and the dataset's ray batches, with the test code unchanged.  The
million-value percentile case and render.py need the MI355X."""

import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(not (shutil.which('clang++') or os.path.exists('/opt/rocm/lib/llvm/bin/clang++')),
                                reason='needs clang++')


def test_render_kernels_pass_on_the_simulator():
  env = dict(os.environ, MNR_TESTS_ON_SIMULATOR='1')
  cmd = [sys.executable, '-m', 'pytest', '-q', '-m', 'gpu', '-p', 'no:cacheprovider', 'tests/test_gpu_render.py', '-k',
         '(kernel or composed or suite or argument_errors or dataset) and not large']
  r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
  tail = '\n'.join((r.stdout + r.stderr).splitlines()[-25:])
  assert r.returncode == 0, tail
  assert ' passed' in tail and 'failed' not in tail and 'skipped' not in tail, tail
