"""BASELINE config 5 from the command line: python tools/replay.py --scans 50000 [--no-lifelong] [--mode async --period 0.025]
[--save-session FILE [--save-at K]] [--load-session FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from slam_toolbox_amd import replay  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scans", type=int, default=5000)
ap.add_argument("--no-lifelong", action="store_true")
ap.add_argument("--mode", default="sync", choices=["sync", "async"])
ap.add_argument("--period", type=float, default=0.025)
ap.add_argument("--progress", type=int, default=0)
ap.add_argument("--save-session", default=None, help="save the mapper (kh_mapper_save) to this file, behind queue scan --save-at")
ap.add_argument("--save-at", type=int, default=None, help="queue scan behind which --save-session saves (default: the last)")
ap.add_argument("--load-session", default=None, help="resume a run saved with --save-session (same --scans) instead of starting empty")
a = ap.parse_args()
out = replay.run(a.scans, lifelong=not a.no_lifelong, mode=a.mode, period_s=a.period, progress=a.progress or None,
                 save_session=a.save_session, save_at=a.save_at, load_session=a.load_session)
out.pop("poses", None); out.pop("alive_queue_index", None)
print(json.dumps(out))
