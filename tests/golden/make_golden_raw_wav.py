#!/usr/bin/env python3
"""tests/golden/raw_wav.json from the REAL reference classes (/root/reference/raw_dataset.py).

The six ``.wav`` classes of the reference are constructed over the synthetic tree of tests/raw_wav_fixture.py and every
item is read.  ``librosa`` / ``soundfile`` are absent here: make_golden.install_shims stubs them, ``find_files`` gets
its documented behaviour (recursive, sorted, as make_golden_dataset.py installs it), and ``torchaudio_load`` - the
waveform read this package replaces by its device decoder - is replaced by a stub, so the files need no content.  What
is stored is data only: each class's length, file order, tag / label tables and the metadata of every item.

Usage:  python tests/golden/make_golden_raw_wav.py
"""
import json
import os
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import torch

import make_golden as mg
import raw_wav_fixture as fx


def main():
    mg.install_shims()
    import librosa

    def find_files(directory, ext=None, recurse=True, case_sensitive=False, limit=None, offset=0):
        exts = [ext] if isinstance(ext, str) else list(ext)
        out = []
        for dp, _, fs in os.walk(directory):
            out += [os.path.join(dp, f) for f in fs if any(f.lower().endswith("." + e.lower()) for e in exts)]
        return sorted(out)

    librosa.util.find_files = find_files
    import raw_dataset as ref
    ref.torchaudio_load = lambda filepath: [torch.zeros(1, 1), 16000]

    golden = {}
    with tempfile.TemporaryDirectory() as root:
        n = fx.build(root, lambda path, k: open(path, "wb").close())
        for name, make in fx.cases(ref, root).items():
            golden[name] = fx.record(make(), root)
            print("  %-60s %d items" % (name, golden[name]["len"]))
    path = os.path.join(HERE, "raw_wav.json")
    with open(path, "w") as f:
        json.dump(golden, f, indent=1, sort_keys=True)
        f.write("\n")
    print("  wrote raw_wav.json (%d files in the tree, %.1f KB)" % (n, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
