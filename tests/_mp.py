"""Helpers for multi-process (torchrun, gloo) tests on the CPU."""
from __future__ import annotations

import os
import re
import socket
import subprocess
import sys
from typing import Dict, List, Optional

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def free_port(span: int = 1) -> int:
    """A port P with P .. P + span - 1 all free right now.  The parameter
    server derives its other listeners from the master port (P + 1: payload
    group, P + 2: payload-mode store), so its tests ask for the whole range:
    a neighbour in use by another process makes rank 0 fail with EADDRINUSE
    and the other ranks wait for it until their timeout."""
    for _ in range(200):
        socks = [socket.socket() for _ in range(span)]
        try:
            socks[0].bind(("127.0.0.1", 0))
            port = socks[0].getsockname()[1]
            if port + span > 65536:
                continue
            for k in range(1, span):
                socks[k].bind(("127.0.0.1", port + k))
            return port
        except OSError:
            continue
        finally:
            for s in socks:
                s.close()
    raise RuntimeError(f"no {span} consecutive free ports found")


def cpu_env(extra: Optional[Dict[str, str]] = None) -> Dict[str, str]:
    env = dict(os.environ)
    env.update({"MASTER_ADDR": "127.0.0.1", "PDRNN_FORCE_CPU": "1", "OMP_NUM_THREADS": "1",
                "PYTHONPATH": ROOT + os.pathsep + env.get("PYTHONPATH", ""),
                "HIP_VISIBLE_DEVICES": "", "CUDA_VISIBLE_DEVICES": ""})
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    if extra:
        env.update(extra)
    return env


def run(cmd: List[str], cwd: str, timeout: float = 240, env=None) -> str:
    p = subprocess.run(cmd, cwd=cwd, env=env or cpu_env(), capture_output=True, text=True, timeout=timeout)
    out = p.stdout + p.stderr
    if p.returncode != 0:
        raise AssertionError(f"{' '.join(cmd)} failed ({p.returncode}):\n{out[-4000:]}")
    return out


def torchrun(script_and_args: List[str], nproc: int, cwd: str, timeout: float = 240, env=None) -> str:
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
           "--master-addr=127.0.0.1", f"--master-port={free_port()}"] + script_and_args
    return run(cmd, cwd, timeout, env)


_BATCH = re.compile(r"Rank: (\d+)\s+Train Batch: (\d+)/(\d+) \(\d+%\)\tLoss: ([\d.]+)\tAcc: (\d+)/(\d+)")


def batch_losses(log: str) -> Dict[int, List[float]]:
    """rank -> per-step losses parsed from the reference-format Train Batch lines."""
    out: Dict[int, List[float]] = {}
    for m in _BATCH.finditer(log):
        out.setdefault(int(m.group(1)), []).append(float(m.group(4)))
    return out
