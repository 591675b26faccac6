"""Build-time guard for the row-split compositing kernels (log_amd/csrc/blend.hip): what the compiler makes of them.

lr_blend_fwd_rows_kernel is built around a two-chunk software pipeline -- the gather of the next chunk's records is in
flight while the current chunk is composited.  Scratch accesses count in the same counter as that gather (vmcnt), so ONE
spilled value that is reloaded inside the chunk loop makes the wave wait for its whole prefetch once per chunk; the kernel
once did exactly that while its source said "no spill" (docs/HISTORY.md, profiles/fwd_rows_prefetch.md).  Nothing on a GPU
shows such a regression except a few per cent of time, so it is held here, on the compiler's own report:

  blend.hip is compiled for gfx950 with log_amd.build's flags, to assembly, with -Rpass-analysis=kernel-resource-usage;
  every instantiation of the two row-split kernels has scratch size 0, no VGPR spill and no scratch_* instruction in its
  body, and an occupancy not below what it was built for (five waves per SIMD; four for the reverse walk without masks).

Only the resource numbers and the scratch mnemonics of these kernels are read.  No GPU is needed; skipped without hipcc."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (kernel, template arguments) -> the least occupancy [waves / SIMD] it is built for
#   lr_blend_fwd_rows_kernel<EXTRAS>, lr_blend_bwd_rows_kernel<MASKS, ABS>
WANT = {
    ("lr_blend_fwd_rows_kernel", (1,)): 5,
    ("lr_blend_fwd_rows_kernel", (0,)): 5,
    ("lr_blend_bwd_rows_kernel", (1, 0)): 5,
    ("lr_blend_bwd_rows_kernel", (1, 1)): 5,
    ("lr_blend_bwd_rows_kernel", (0, 0)): 4,
    ("lr_blend_bwd_rows_kernel", (0, 1)): 4,
}


def _kernel_of(mangled):
    """_Z24lr_blend_fwd_rows_kernelILb1EEv... -> ("lr_blend_fwd_rows_kernel", (1,)); None for anything else."""
    m = re.match(r"_Z\d+(lr_blend_(?:fwd|bwd)_rows_kernel)I((?:Lb[01]E)+)E", mangled)
    return (m.group(1), tuple(int(b) for b in re.findall(r"Lb([01])E", m.group(2)))) if m else None


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """-> (resources {kernel: {field: text}}, bodies {kernel: [assembly lines]}) of one compilation of blend.hip."""
    from log_amd import build
    if not os.path.exists(build.HIPCC):
        pytest.skip("no hipcc at %s" % build.HIPCC)
    asm = str(tmp_path_factory.mktemp("blend_isa") / "blend.s")
    p = subprocess.run([build.HIPCC] + build.FLAGS + ["-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                                                      os.path.join(build.CSRC, "blend.hip"), "-o", asm],
                       capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-4000:]
    resources, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?)\s*\[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        key, _, value = m.group(1).rpartition(":")
        if key.strip() == "Function Name":
            cur = _kernel_of(value.strip())
            if cur is not None:
                resources[cur] = {}
        elif cur is not None:
            resources[cur][key.strip()] = value.strip()
    bodies, cur = {}, None
    for line in open(asm):
        m = re.match(r"(_Z\w+):", line)
        if m:
            cur = _kernel_of(m.group(1))
            if cur is not None:
                bodies[cur] = []
        elif line.startswith(".Lfunc_end"):                     # (a kernel's text: from its label to its .Lfunc_end)
            cur = None
        elif cur is not None:
            bodies[cur].append(line)
    return resources, bodies


def test_every_row_split_kernel_is_reported(compiled):
    resources, bodies = compiled
    assert set(resources) == set(WANT), sorted(set(resources) ^ set(WANT))
    assert set(bodies) == set(WANT), sorted(set(bodies) ^ set(WANT))
    for k, body in bodies.items():
        assert sum(1 for l in body if re.match(r"\s+v_\w+", l)) > 200, (k, len(body))       # a whole kernel, not a stub


@pytest.mark.parametrize("kernel", sorted(WANT), ids=lambda k: "%s<%s>" % (k[0], ",".join(map(str, k[1]))))
def test_no_scratch_at_the_occupancy_built_for(compiled, kernel):
    resources, bodies = compiled
    r = resources[kernel]
    print("%s<%s>: %s VGPRs, %s AGPRs, %s SGPRs, scratch %s B/lane, occupancy %s" % (
        kernel[0], ",".join(map(str, kernel[1])), r["VGPRs"], r["AGPRs"], r["TotalSGPRs"], r["ScratchSize [bytes/lane]"],
        r["Occupancy [waves/SIMD]"]))
    assert int(r["ScratchSize [bytes/lane]"]) == 0, r
    assert int(r["VGPRs Spill"]) == 0 and r["Dynamic Stack"] == "False", r
    assert int(r["Occupancy [waves/SIMD]"]) >= WANT[kernel], r
    scratch = [l.strip() for l in bodies[kernel] if re.match(r"\s+scratch_\w+", l)]
    assert not scratch, scratch[:8]
