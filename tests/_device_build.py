"""The device-only compile of rl_api.hip with the library's own flags (hipcc cross-compiles without a GPU), made once per pytest
process and shared by the tests that read the kernels' resources or instructions: one compile takes about two minutes.  The
*_abi.py modules import the fixture `kernels` and variant_of_name by name."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "robigo_luculenta_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

_build = None


def device_build():
    """(assembly text, {kernel: its .amdgpu_metadata integers}, {kernel: its kernel-resource-usage remarks}); skips without hipcc."""
    global _build
    if _build is not None:
        return _build
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc")
    make = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^FLAGS = (.*?)\n(?!\s)", make, re.S | re.M).group(1).replace("\\\n", " ")
    flags = flags.replace("$(ARCH)", "gfx950").replace("$(EXTRA)", "").split()
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "k.s")
        run = subprocess.run([HIPCC] + flags + ["-DRL_BUILD_ID=\"x\"", "--cuda-device-only", "-S", "-o", asm, "rl_api.hip",
                                                "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, capture_output=True, timeout=900)
        assert run.returncode == 0, run.stderr.decode()[-2000:]
        text = open(asm).read()
    remarks, name = {}, None
    for line in run.stderr.decode().splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            remarks[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[", line)
        if m and name:
            remarks[name][m.group(1).strip()] = int(m.group(2))
    assert remarks, run.stderr.decode()[-2000:]
    metadata = {}
    for entry in re.split(r"\n  - ", text[text.index(".amdgpu_metadata"):]):
        m = re.search(r"^\s+\.name:\s+(\S+)$", entry, re.M)
        if m:
            metadata[m.group(1)] = {k: int(v) for k, v in re.findall(r"^\s+\.(\w+):\s+(\d+)$", entry, re.M)}
            metadata[m.group(1)]["dynamic_stack"] = int(bool(re.search(r"^\s+\.uses_dynamic_stack:\s+true", entry, re.M)))
    _build = (text, metadata, remarks)
    return _build


@pytest.fixture(scope="module")
def kernels():
    """Metadata of every kernel from the device-only -S compile with the library's own flags."""
    return device_build()[1]


def variant_of_name(name, kernel):
    """(stage, cyl), each a one-digit string, of the instantiation kernel<stage, cyl> that the mangled `name` is."""
    return re.search(kernel + r"ILi([012])ELb([01])E", name).groups()
