#!/usr/bin/env python
"""SHA-256 digests of the CPU HEVC encoder's streams with EncoderConfig.hevc_intra_split 0 and 1
(tests/hevc_intra4_content.py split_digests): run at the commit whose streams are to be pinned, it
writes tests/golden/hevc_intra_split_parent.json, which tests/test_hevc_intra4.py reproduces.

    python tools/gen_hevc_intra_split_digests.py [--out tests/golden/hevc_intra_split_parent.json]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "hevc_intra_split_parent.json"))
    a = ap.parse_args()
    from mxdesk import native
    from tests.hevc_intra4_content import split_digests

    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(split_digests(native()), indent=1, sort_keys=True) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
