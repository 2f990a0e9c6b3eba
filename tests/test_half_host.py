"""CPU tests of the 16-bit (fp16 / bf16) output path: the header's new enums, evam_pp_norm_table (the very table the
device reads, evam_pp_run fills its descriptor block from the same function) against the oracle's fp32 table narrowed
by torch, and the opt-in pairing of a 16-bit output tensor with ``PreProcInfo.precision``.

Expected 16-bit values everywhere: ``torch.from_numpy(fp32 reference).to(torch.float16 | torch.bfloat16)``, compared
bitwise as int16."""
import ctypes
import os
import re
import weakref

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "evam_pp.h")

# flags (1 range, 2 mean/std), range, mean, std
NORM_A = (3, (0.0, 1.0), (0.406, 0.456, 0.485), (0.225, 0.224, 0.229))
NORM_NONE = (0, (0.0, 255.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
CONFIGS = {
    "imagenet": NORM_A,
    "none": NORM_NONE,
    "range_pm1": (1, (-1.0, 1.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
    "tiny_range": (1, (0.0, 1e-5), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),    # fp16: 765 of 768 entries subnormal
    "tiny_std": (2, (0.0, 255.0), (0.0, 0.0, 0.0), (1e-3, 3e-3, 1.0)),   # fp16: 249 entries +inf
}


def c_cfg(N, dtype, flags, rng_, mean, std):
    c = N.EvamPreproc()
    c.out_dtype, c.norm_flags = dtype, flags
    c.range[0], c.range[1] = rng_
    for i in range(3):
        c.mean[i], c.std[i] = mean[i], std[i]
    return c


def narrowed(torch, ref32, tdt):
    """fp32 numpy array -> its torch cast to the 16-bit dtype, as int16 bits."""
    return torch.from_numpy(np.ascontiguousarray(ref32)).to(tdt).view(torch.int16).numpy()


def test_header_enums_and_abi_version(evam):
    src = open(HEADER).read()
    vals = {k: int(v, 0) for k, v in re.findall(r"(EVAM_\w+)\s*=\s*(-?0x[0-9A-Fa-f]+|-?\d+)", src)}
    N = evam.native
    assert (vals["EVAM_DTYPE_U8"], vals["EVAM_DTYPE_F32"]) == (N.DTYPE_U8, N.DTYPE_F32) == (0, 1)
    assert (vals["EVAM_DTYPE_F16"], vals["EVAM_DTYPE_BF16"]) == (N.DTYPE_F16, N.DTYPE_BF16) == (2, 3)
    assert re.search(r"#define\s+EVAM_PP_ABI_VERSION\s+3\b", src)
    assert N.ABI_VERSION == 3 and evam.load_library().evam_pp_abi_version() == 3
    assert "evam_pp_norm_table" in N.EXPORTED_SYMBOLS


@pytest.mark.parametrize("name", list(CONFIGS))
def test_norm_table_matches_oracle(evam, O, name):
    import torch

    N = evam.native
    lib = evam.load_library()
    flags, rng_, mean, std = CONFIGS[name]
    ref = O.np_norm_lut(flags, rng_, mean, std)
    got32 = np.zeros((3, 256), np.float32)
    assert lib.evam_pp_norm_table(ctypes.byref(c_cfg(N, N.DTYPE_F32, *CONFIGS[name])), got32.ctypes.data) == 0
    assert np.array_equal(got32.view(np.uint32), ref.view(np.uint32)), name
    for dt, tdt in ((N.DTYPE_F16, torch.float16), (N.DTYPE_BF16, torch.bfloat16)):
        got = np.full((3, 256), 0x5555, np.int16)
        assert lib.evam_pp_norm_table(ctypes.byref(c_cfg(N, dt, *CONFIGS[name])), got.ctypes.data) == 0
        want = narrowed(torch, ref, tdt)
        bad = np.argwhere(got != want)
        assert not len(bad), f"{name} {tdt}: {len(bad)} entries differ, first {bad[0]}: " \
                             f"{got[tuple(bad[0])] & 0xFFFF:#06x} != {want[tuple(bad[0])] & 0xFFFF:#06x}"
    # the cases these configs are here for
    h = narrowed(torch, ref, torch.float16).view(np.uint16)
    if name == "tiny_range":
        assert int(((h & 0x7C00) == 0).sum() - ((h & 0x7FFF) == 0).sum()) == 765
    if name == "tiny_std":
        assert int((h == 0x7C00).sum()) == 249
    if name in ("imagenet", "none"):  # the pixel-parity normalisations: 256 distinct 16-bit values per channel
        for tdt in (torch.float16, torch.bfloat16):
            assert all(len(set(row.tolist())) == 256 for row in narrowed(torch, ref, tdt))


def test_norm_table_narrowing_edges(evam):
    """The fp32 -> 16-bit narrowing over ties, subnormals, overflow, infinities and signed zero, driven through the
    table: a chosen fp32 value is put into an entry exactly and the 16-bit entry compared with torch's cast of it."""
    import torch

    N = evam.native
    lib = evam.load_library()
    vals = np.array([0.0, -0.0, 1.0, -1.0, 65504.0, 65519.996, 65520.0, 65536.0, -65520.0, 1e38, 3.4028235e38,
                     2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.0000001, 2.0 ** -26, 1.5 * 2.0 ** -24,
                     2.5 * 2.0 ** -24, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -20,
                     2047.0 / 2048 * 2.0 ** -14, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20,
                     float("inf"), float("-inf"), 1e-45, -1e-40, 0.1, 255.0 / 0.229], np.float32)
    for v in vals:
        if v == 0:  # the carrier below gives +0 for either zero; the sign of zero is checked after the loop
            continue
        for dt, tdt in ((N.DTYPE_F16, torch.float16), (N.DTYPE_BF16, torch.bfloat16)):
            # an exact carrier: entry [c][0] = (0 - mean[c]) / 1 with mean[c] = -v is v itself
            c = c_cfg(N, dt, 2, (0.0, 255.0), (-float(v),) * 3, (1.0, 1.0, 1.0))
            got = np.zeros((3, 256), np.int16)
            assert lib.evam_pp_norm_table(ctypes.byref(c), got.ctypes.data) == 0
            want = narrowed(torch, np.array([v], np.float32), tdt)[0]
            assert got[0, 0] == want, f"{float(v)!r} {tdt}: {got[0, 0] & 0xFFFF:#06x} != {want & 0xFFFF:#06x}"
    # the sign of zero: u = 0 divided by a negative std is -0.0 in fp32 and stays -0 in both types
    for dt in (N.DTYPE_F16, N.DTYPE_BF16):
        c = c_cfg(N, dt, 2, (0.0, 255.0), (0.0, 0.0, 0.0), (-1.0, 1.0, 1.0))
        got = np.zeros((3, 256), np.uint16)
        assert lib.evam_pp_norm_table(ctypes.byref(c), got.ctypes.data) == 0
        assert got[0, 0] == 0x8000 and got[1, 0] == 0x0000


def test_norm_table_errors(evam):
    N = evam.native
    lib = evam.load_library()
    buf = np.zeros(768, np.float32)
    assert lib.evam_pp_norm_table(ctypes.byref(c_cfg(N, N.DTYPE_U8, *NORM_A)), buf.ctypes.data) == N.ERR_INVALID_ARG
    for dt in (N.DTYPE_F32, N.DTYPE_F16, N.DTYPE_BF16):
        c = c_cfg(N, dt, 3, (0.0, 1.0), (0.0, 0.0, 0.0), (1.0, 0.0, 1.0))
        assert lib.evam_pp_norm_table(ctypes.byref(c), buf.ctypes.data) == N.ERR_INVALID_ARG
        assert b"std[1]" in lib.evam_pp_last_error()
    assert lib.evam_pp_norm_table(ctypes.byref(c_cfg(N, 4, *NORM_A)), buf.ctypes.data) == N.ERR_UNSUPPORTED
    assert lib.evam_pp_norm_table(None, buf.ctypes.data) == N.ERR_INVALID_ARG
    assert lib.evam_pp_norm_table(ctypes.byref(c_cfg(N, N.DTYPE_F16, *NORM_A)), None) == N.ERR_INVALID_ARG


def test_output_dtype_pairing(evam):
    import torch

    N = evam.native
    PI = evam.PreProcInfo
    t = {d: torch.empty(1, 3, 2, 2, dtype=d) for d in (torch.uint8, torch.float32, torch.float16, torch.bfloat16)}
    # uint8 and float32 behave as before, whatever insignificant precision is stated
    for prec in (None, "FP32", "U8", "fp16", "INT8", 16):
        assert evam.output_dtype(t[torch.uint8], PI(precision=prec)) == N.DTYPE_U8
        assert evam.output_dtype(t[torch.float32], PI(precision=prec)) == N.DTYPE_F32
    assert evam.output_dtype(t[torch.float32], None) == N.DTYPE_F32
    # matched
    assert evam.output_dtype(t[torch.float16], PI(precision="FP16")) == N.DTYPE_F16 == 2
    assert evam.output_dtype(t[torch.bfloat16], PI(precision="BF16")) == N.DTYPE_BF16 == 3
    # a 16-bit tensor whose precision does not name its type: ERR_UNSUPPORTED, and the message says what to state
    for d, prec in ((torch.float16, None), (torch.float16, "BF16"), (torch.float16, "FP32"), (torch.bfloat16, None),
                    (torch.bfloat16, "FP16")):
        with pytest.raises(evam.PreProcError) as ei:
            evam.output_dtype(t[d], PI(precision=prec))
        assert ei.value.status == N.ERR_UNSUPPORTED and "precision" in str(ei.value)
    with pytest.raises(evam.PreProcError) as ei:
        evam.output_dtype(t[torch.float16], None)
    assert ei.value.status == N.ERR_UNSUPPORTED
    # precision FP16 / BF16 with a tensor of any other dtype: ERR_INVALID_ARG
    for d, prec in ((torch.float32, "FP16"), (torch.uint8, "FP16"), (torch.float32, "BF16"), (torch.uint8, "BF16")):
        with pytest.raises(evam.PreProcError) as ei:
            evam.output_dtype(t[d], PI(precision=prec))
        assert ei.value.status == N.ERR_INVALID_ARG
    with pytest.raises(evam.PreProcError) as ei:
        evam.output_dtype(torch.empty(1, 3, 2, 2, dtype=torch.float64), PI())
    assert ei.value.status == N.ERR_UNSUPPORTED


def test_convert_pairs_dtype_and_follows_precision(evam):
    """HipPreProcessor.convert on CPU tensors (a recording stand-in for evam_pp_run, the device check skipped): the C
    config carries out_dtype 2 / 3 when tensor and precision match, the three pairing rules hold, and the per-tensor and
    per-config caches follow a change of ``info.precision`` between calls."""
    import torch

    N = evam.native
    calls = []

    class Rec(evam.HipPreProcessor):
        def _check_device(self, out):  # CPU tensors here
            pass

    def fake_run(h, arr, n_srcs, items, n_items, cfg, tref, xf):
        calls.append((cfg._obj.out_dtype, tref._obj.data, tuple(cfg._obj.mean)))
        return 0

    pp = Rec.__new__(Rec)
    pp._torch, pp.device, pp._h = torch, 0, None
    pp._tdesc, pp._cfg_cache, pp._last_cfg = {}, {}, None
    pp._default_info = evam.PreProcInfo()
    pp._run, pp._bind_stream = fake_run, lambda: None
    batch = evam.ImageBatch.__new__(evam.ImageBatch)
    batch.images, batch.c_array = [None], (N.EvamImage * 1)()

    h16, b16 = torch.empty(2, 3, 8, 8, dtype=torch.float16), torch.empty(2, 3, 8, 8, dtype=torch.bfloat16)
    f32, u8 = torch.empty(2, 3, 8, 8), torch.empty(2, 3, 8, 8, dtype=torch.uint8)
    info = evam.PreProcInfo(mean=(1.0, 2.0, 3.0), std=(1.0, 1.0, 1.0), precision="FP16")
    pp.convert(batch, h16, info)
    pp.convert(batch, h16, info)  # the identity fast path
    assert [c[0] for c in calls] == [N.DTYPE_F16, N.DTYPE_F16] and calls[-1][1] == h16.data_ptr()

    def refused(out, inf, status):
        n = len(calls)
        with pytest.raises(evam.PreProcError) as ei:
            pp.convert(batch, out, inf)
        assert ei.value.status == status and len(calls) == n, str(ei.value)
        return str(ei.value)

    # flipping the precision of the same info object between calls is followed, in every direction
    info.precision = "BF16"
    refused(h16, info, N.ERR_UNSUPPORTED)
    pp.convert(batch, b16, info)
    assert calls[-1][0] == N.DTYPE_BF16 == 3 and calls[-1][1] == b16.data_ptr()
    refused(f32, info, N.ERR_INVALID_ARG)
    refused(u8, info, N.ERR_INVALID_ARG)
    info.precision = None
    assert "precision" in refused(h16, info, N.ERR_UNSUPPORTED)
    refused(b16, info, N.ERR_UNSUPPORTED)
    pp.convert(batch, f32, info)
    assert calls[-1][0] == N.DTYPE_F32
    pp.convert(batch, u8, info)
    assert calls[-1][0] == N.DTYPE_U8
    info.precision = "FP16"
    refused(f32, info, N.ERR_INVALID_ARG)
    pp.convert(batch, h16, info)
    assert calls[-1][0] == N.DTYPE_F16 == 2 and calls[-1][2] == (1.0, 2.0, 3.0)
    info.precision = "FP32"  # not significant: as None
    pp.convert(batch, f32, info)
    assert calls[-1][0] == N.DTYPE_F32
    refused(h16, info, N.ERR_UNSUPPORTED)
    # no info at all: the default has no precision
    refused(h16, None, N.ERR_UNSUPPORTED)
    # a second info object with the other precision, alternating with the first
    other = evam.PreProcInfo(mean=(1.0, 2.0, 3.0), std=(1.0, 1.0, 1.0), precision="BF16")
    info.precision = "FP16"
    for _ in range(2):
        pp.convert(batch, h16, info)
        pp.convert(batch, b16, other)
        assert (calls[-2][0], calls[-1][0]) == (N.DTYPE_F16, N.DTYPE_BF16)
    assert weakref.ref(h16)() is h16  # the tensors outlived their cached descriptors


def test_from_model_proc_reads_precision(evam):
    PI = evam.PreProcInfo
    assert PI.from_model_proc(None).precision is None
    assert PI.from_model_proc({"format": "image", "params": {"resize": "aspect-ratio"}}).precision is None
    assert PI.from_model_proc({"format": "image", "precision": "FP16", "params": {}}).precision == "FP16"
    assert PI.from_model_proc({"format": "image", "params": {"precision": "BF16"}}).precision == "BF16"
    assert PI.from_model_proc({"precision": "FP16", "range": [0, 1]}).precision == "FP16"  # a bare params dict
    assert PI.from_model_proc({"format": "image", "precision": "U8", "params": {}}).precision == "U8"  # kept, not significant
    N = evam.native
    # the precision does not reach the C struct except through the dtype code
    a = PI(range=(0.0, 1.0), precision="FP16").to_c(N.DTYPE_F16)
    b = PI(range=(0.0, 1.0)).to_c(N.DTYPE_F16)
    assert bytes(a) == bytes(b) and a.out_dtype == N.DTYPE_F16


def test_inference_model_out_dtype_sets_precision(evam):
    ps = evam.pipeline_server
    proc = {"input_preproc": [{"format": "image", "precision": "FP16", "params": {"color_space": "RGB"}}]}
    assert ps.InferenceModel(None, (8, 8), out_dtype="f16").preproc_info().precision == "FP16"
    assert ps.InferenceModel(None, (8, 8), out_dtype="bf16").preproc_info().precision == "BF16"
    assert ps.InferenceModel(None, (8, 8)).preproc_info().precision is None
    assert ps.InferenceModel(None, (8, 8), out_dtype="u8").preproc_info().precision is None
    # the blob's type is the model's out_dtype: an fp32 blob stays valid under a model-proc that states FP16
    i = ps.InferenceModel(None, (8, 8), proc).preproc_info()
    assert i.precision is None and i.color_space == "RGB"
    assert ps.InferenceModel(None, (8, 8), proc, out_dtype="bf16").preproc_info().precision == "BF16"
