"""A dependency-free stand-in for torch.utils.tensorboard.SummaryWriter where tensorboard is not installed: the writer contract of the
models (`add_scalar(tag, value, step)`, `add_histogram(tag, values, step)`, `close()`) on one JSON line per call."""
import json
import math
import os


def _number(v):
    """a Python float from a float, a numpy scalar or a one-element tensor (one read-back for a device tensor)"""
    return float(v.item()) if hasattr(v, "item") else float(v)


class ScalarLog:
    """`ScalarLog(path)`: path a file, or a directory (an existing one, or a name without an extension -- as SummaryWriter's log_dir),
    in which `scalars.jsonl` is written.  Lines: {"tag", "step", "value"} for a scalar; {"tag", "step", "min", "mean", "max", "count"} for a
    histogram, which is reduced to those four numbers.  Non-finite values are written as null (JSON has no NaN) -- read() turns them
    back into NaN."""

    def __init__(self, path):
        path = os.fspath(path)
        if os.path.isdir(path) or not os.path.splitext(path)[1]:
            os.makedirs(path, exist_ok=True)
            path = os.path.join(path, "scalars.jsonl")
        elif os.path.dirname(path):
            os.makedirs(os.path.dirname(path), exist_ok=True)
        self.path = path
        self._f = open(path, "a")

    @staticmethod
    def _json(v):
        return v if math.isfinite(v) else None

    def _write(self, rec):
        self._f.write(json.dumps(rec) + "\n")

    def add_scalar(self, tag, scalar_value, global_step=None):
        self._write({"tag": tag, "step": global_step, "value": self._json(_number(scalar_value))})

    def add_histogram(self, tag, values, global_step=None):
        if hasattr(values, "detach"):
            v = values.detach().float().reshape(-1)
            n = int(v.numel())
            import torch
            lo, mean, hi = (float("nan"),) * 3 if n == 0 else torch.stack([v.min(), v.mean(), v.max()]).tolist()     # (one read-back)
        else:
            v = [float(t) for t in values]
            n = len(v)
            lo, mean, hi = (float("nan"),) * 3 if n == 0 else (min(v), sum(v) / n, max(v))
        self._write({"tag": tag, "step": global_step, "min": self._json(lo), "mean": self._json(mean), "max": self._json(hi), "count": n})

    def flush(self):
        self._f.flush()

    def close(self):
        if not self._f.closed:
            self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @staticmethod
    def read(path):
        """the records of a log file, null values back as NaN"""
        with open(path) as f:
            recs = [json.loads(line) for line in f if line.strip()]
        for r in recs:
            for key in ("value", "min", "mean", "max"):
                if key in r and r[key] is None:
                    r[key] = float("nan")
        return recs
