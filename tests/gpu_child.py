"""One child process per set of environment switches, for GPU tests whose library reads its switches once per process
(tests/test_gpu_wgrad_kernels.py).  The rules are those of tests/test_gpu_conv_kernels.py: the parent hands the inputs over in an
.npz and the jobs in a .json, the child writes an .npz; every child has a time limit of its own and is never started twice; a
child that ends by a signal, an abort or its time limit bars every later child of the same runner: a card that has just faulted
gets no further work from here."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest


class ChildRunner:
    def __init__(self, script, strip):
        """script: the file to start with --child IN JOBS OUT; strip(name) -> whether an inherited environment variable is dropped"""
        self.script, self.strip = os.path.abspath(script), strip
        self.dead = ""         # why no further child may start

    def run(self, tmp_path, tag, env, arrays, jobs, timeout):
        """-> (the child's .npz, lazily loaded; its path).  The caller closes the one and removes the other"""
        in_path, job_path, out_path = (str(tmp_path / ("%s_%s" % (tag, s))) for s in ("in.npz", "jobs.json", "out.npz"))
        if self.dead:
            pytest.fail("not started: an earlier child of this module died abnormally (%s); nothing more runs on that GPU" % self.dead,
                        pytrace=False)
        np.savez(in_path, **arrays)
        with open(job_path, "w") as f:
            json.dump(jobs, f)
        e = {k: v for k, v in os.environ.items() if not self.strip(k)}
        e.update(env)
        try:
            r = subprocess.run([sys.executable, self.script, "--child", in_path, job_path, out_path], env=e, capture_output=True, text=True,
                               timeout=timeout)
        except subprocess.TimeoutExpired as ex:
            self.dead = "switch set %s: no end after %d s" % (tag, ex.timeout)
            pytest.fail(self.dead, pytrace=False)
        finally:
            os.remove(in_path)
        if r.returncode != 0:
            # 1: a Python exception, the process itself ended in order.  Anything else (a signal, an abort, a GPU fault) bars every
            # later child, and so does an exception that reports a fault of the GPU
            if r.returncode != 1 or "illegal memory access" in r.stderr or "hipErrorLaunchFailure" in r.stderr:
                self.dead = "switch set %s: exit status %d" % (tag, r.returncode)
            pytest.fail("child of switch set %s ended with status %d:\n%s" % (tag, r.returncode, r.stderr[-3000:]), pytrace=False)
        return np.load(out_path), out_path
