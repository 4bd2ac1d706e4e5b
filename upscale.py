#!/usr/bin/env python
"""Upscale video files 4x on an MI355X:  python upscale.py -i clip.y4m -o results --pretrained DIR  (see uav/cli.py)."""
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "upscale-a-video_amd"))

from uav.cli import main  # noqa: E402

if __name__ == "__main__":
    sys.exit(main())
