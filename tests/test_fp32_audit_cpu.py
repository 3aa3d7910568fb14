"""The float32 arithmetic mode (CS_FLAG_FP32, csrc/gemm_f32.h) AS BUILT, no GPU needed: the flag's value is the same in the C header
and in the ctypes binding, and every kernel of the float32 path is in the gfx950 code object, contracts on the f32-input MFMA, carries
no bf16 instruction (no bf16 MFMA, no bf16 convert) and has no private segment (zero scratch)."""
import importlib.util
import os
import re
import struct
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"

# every kernel the float32 path launches (climsim_hip.hip: run_forward_f32 / run_backward_f32), by mangled name
F32_KERNELS = (
    ["_Z19k_prepare_input_f32PKfPKllliiS0_S0_iPf"]
    + [f"_Z10k_gemm_f32ILi{epi}ELb{wt}ELi{t}ELi{t}EEv7GemmF32" for epi, wt in ((0, 0), (1, 0), (2, 1)) for t in (128, 64)]
    + [f"_Z11k_wgrad_f32ILi{t}EEv12WgradF32Args" for t in (128, 64)]
)
MFMA_F32 = re.compile(r"\bv_mfma_f32_(32x32x2|16x16x4)_f32\b")
BF16 = re.compile(r"\bv_mfma\w*bf16\w*|\bv_cvt\w*bf16\w*|\bv_dot\w*bf16\w*")


def _audit_tool():
    spec = importlib.util.spec_from_file_location("chainw_audit", os.path.join(REPO, "tools", "chainw_audit.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _bodies(listing):
    """mangled name -> instruction lines of every function of an llvm-objdump listing"""
    out, cur = {}, None
    for line in listing.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\w+)>:", line)
        if m:
            cur = m.group(1)
            out[cur] = []
        elif cur:
            out[cur].append(line.split("//")[0])
    return out


def _private_segment_by_kernel(so_path, tmp_path):
    """kernel name -> .private_segment_fixed_size, from the gfx950 code object's metadata note (one map per kernel)"""
    d = open(so_path, "rb").read()
    i = d.find(b"__CLANG_OFFLOAD_BUNDLE__")
    assert i >= 0, "no offload bundle in " + so_path
    n = struct.unpack_from("<Q", d, i + 24)[0]
    off, blob = i + 32, None
    for _ in range(n):
        o, sz, tl = struct.unpack_from("<QQQ", d, off)
        off += 24
        if "gfx950" in d[off:off + tl].decode():
            blob = d[i + o:i + o + sz]
        off += tl
    assert blob, "no gfx950 code object in " + so_path
    co = tmp_path / "gfx950.co"
    co.write_bytes(blob)
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True, check=True).stdout
    out = {}
    for chunk in re.split(r"\n\s{2}- ", notes):
        name = re.search(r"^\s*\.name:\s+(\S+)", chunk, re.M)
        priv = re.search(r"^\s*\.private_segment_fixed_size:\s+(\d+)", chunk, re.M)
        if name and priv:
            out[name.group(1)] = int(priv.group(1))
    return out


def test_flag_value_matches_the_header():
    from climsim_amd import _lib
    hdr = open(os.path.join(REPO, "include", "climsim_hip.h")).read()
    m = re.search(r"#define\s+CS_FLAG_FP32\s+(\d+)", hdr)
    assert m and int(m.group(1)) == _lib.CS_FLAG_FP32 == 1024
    used = [int(v) for v in re.findall(r"#define\s+CS_FLAG_\w+\s+(\d+)", hdr) if int(v) != 1024]
    assert all(v & 1024 == 0 for v in used)                    # a bit of its own


def test_float32_kernels_use_f32_mfma_only_and_no_scratch(tmp_path):
    from climsim_amd import build as b
    lib = b.build()
    bodies = _bodies(_audit_tool().disassemble(lib))
    priv = _private_segment_by_kernel(lib, tmp_path)
    for k in F32_KERNELS:
        assert k in bodies, f"{k} missing from the code object"
        text = "\n".join(bodies[k])
        if "gemm" in k or "wgrad" in k:
            assert MFMA_F32.search(text), f"{k}: no f32-input MFMA"
        bad = BF16.findall(text)
        assert not bad, f"{k}: bf16 instructions {sorted(set(bad))[:5]}"
        assert k in priv, f"{k}: no metadata"
        assert priv[k] == 0, f"{k}: private segment of {priv[k]} bytes"
