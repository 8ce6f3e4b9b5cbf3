"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol the
header declares, the module API / state_dict schema matches the reference, and the
product path refuses to run without the GPU (no silent fallback)."""
import ctypes
import re

import numpy as np
import pytest
import torch

from vdn_hip import images, lib
from vdn_train import synth, factory


def test_library_exports_every_declared_symbol():
    l = lib.load()
    text = open(lib.HEADER).read()
    declared = re.findall(r"\bint\s+(vdn_\w+)\s*\(", text)
    assert len(declared) >= 10
    for name in declared:
        assert hasattr(l, name), name
    assert l.vdn_abi_version() == int(re.search(r"#define\s+VDN_ABI_VERSION\s+(\d+)", text).group(1)) == 28


def test_struct_layouts_are_c_layouts():
    assert ctypes.sizeof(lib.VdnChunkDesc) == 112 and lib.struct_dtype("VdnChunkDesc").itemsize == 112
    assert ctypes.sizeof(lib.VdnWeightNormDesc) == 40
    # {const float*, double, int32 (+4 pad), 7 pointers}: the double and the 1-byte pointer target do not change C's layout rules
    assert ctypes.sizeof(lib.VdnMeshMcArgs) == 8 + 8 + 8 + 7 * 8 and lib.VdnMeshMcArgs.isovalue.offset == 8 and lib.VdnMeshMcArgs.cube_case.offset == 24


def test_argument_errors_are_reported_not_ignored():
    a = lib.VdnSdfArgs()
    with pytest.raises(lib.VdnError):
        lib.call("vdn_sdf_mlp_fwd_f32", 0, a, None)       # P == 0 / null blob -> status < 0, never reaches the GPU
    with pytest.raises(lib.VdnError):
        lib.call("vdn_merge_sorted", lib.VdnMergeArgs(), None)
    # this round's entry points: empty argument blocks / null pointers are refused before anything is launched
    c, b, s = lib.VdnCompositeArgs(), lib.VdnCompositeBwdArgs(), lib.VdnSdfArgs()
    for name, args in (("vdn_shade_fused_bf16", (s, None, 1, c, None, None)),
                       ("vdn_sdf_fwd_tail_bf16", (s, None)),
                       ("vdn_feat_composite", (c, None)),
                       ("vdn_composite_train", (c, b, None, None, None, 0.1, 1.0, None)),
                       ("vdn_composite_fwd_train", (c, None, None, 1.0, 1.0, None)),
                       ("vdn_composite_bwd_train", (b, None, None, None, None, 0.1, 1.0, None)),
                       ("vdn_mesh_mc_count", (lib.VdnMeshMcArgs(), None)),
                       ("vdn_mesh_mc_emit", (lib.VdnMeshMcArgs(), None)),
                       ("vdn_eikonal_reduce", (None, 0, None, None))):
        with pytest.raises(lib.VdnError):
            lib.call(name, *args)


def test_state_dict_schema_and_param_counts():
    rend = factory.build_renderer(wdepth=True, device="cpu")
    sd = rend.sdf_network.state_dict()
    assert list(sd)[:3] == ["lin0.bias", "lin0.weight_g", "lin0.weight_v"]
    assert sd["lin3.weight_v"].shape == (217, 256) and sd["lin4.weight_v"].shape == (256, 256)
    assert sd["lin8.weight_g"].shape == (257, 1) and sd["lin0.weight_v"].shape == (256, 39)
    count = lambda m: sum(p.numel() for p in m.parameters())
    assert count(rend.sdf_network) == 529076 and count(rend.color_network) == 273414
    assert count(rend.depth_network) == 297408 and count(rend.nerf) == 618980
    assert list(rend.deviation_network.state_dict()) == ["variance"]
    nk = list(rend.nerf.state_dict())
    assert nk[:2] == ["pts_linears.0.weight", "pts_linears.0.bias"] and "dpt_linear.weight" in nk
    assert rend.nerf.state_dict()["pts_linears.5.weight"].shape == (256, 340)
    total = sum(count(m) for m in (rend.nerf, rend.sdf_network, rend.deviation_network, rend.color_network))
    assert total - 12384 == 1409087          # SURVEY.md 8e all-reduce payload (womsk_white has no dpt head)


def test_synth_states_load_into_modules_and_roundtrip():
    st = synth.make_all_states(0, wdepth=True)
    rend = factory.build_renderer(wdepth=True, device="cpu", states=st)
    for k, v in st["sdf_network_fine"].items():
        assert np.array_equal(rend.sdf_network.state_dict()[k].numpy(), v)
    rend.nerf.load_state_dict({k: torch.as_tensor(v) for k, v in synth.make_nerf_state(0).items()}, strict=False)


def test_geometric_init_matches_reference_statistics():
    torch.manual_seed(0)
    from dpt_models.fields import SDFNetwork
    net = SDFNetwork(**factory.CONF["sdf_network"])
    sd = net.state_dict()
    assert torch.all(sd["lin8.bias"] == -0.5) and torch.all(sd["lin0.weight_v"][:, 3:] == 0)
    assert abs(sd["lin8.weight_v"].mean().item() - np.sqrt(np.pi) / 16) < 1e-4
    assert torch.all(sd["lin4.weight_v"][:, -36:] == 0)
    assert torch.allclose(sd["lin2.weight_g"][:, 0], sd["lin2.weight_v"].norm(dim=1))


def test_no_cpu_fallback():
    rend = factory.build_renderer(wdepth=False, device="cpu")
    with pytest.raises(RuntimeError):
        rend.sdf_network.sdf(torch.zeros(4, 3))
    with pytest.raises(RuntimeError):
        rend.render(torch.zeros(2, 3), torch.zeros(2, 3), torch.zeros(2, 1), torch.ones(2, 1))


def test_unsupported_shapes_raise():
    from dpt_models.fields import SDFNetwork, RenderingNetwork
    with pytest.raises(ValueError):
        images.sdf_streams(3, 257, 128, 8, (4,), 6)
    with pytest.raises(ValueError):
        images.rendering_streams(256, "no_view_dir", 9, 3, 256, 4, 4)
    with pytest.raises(ValueError):
        factory.build_renderer(device="cpu", n_importance=62)


def test_renderer_level_precision_switch(monkeypatch):
    """One setting puts all four networks of a renderer on the bf16 kernels: the constructor keyword, the VDN_PRECISION environment
    default an unchanged dpt_runner.py picks up, or the `precision` property. The reference's positional signature
    (renderer.py:78-88) is untouched: without any of them the networks stay on the fp32 parity kernels."""
    from dpt_models.renderer import NeuSRenderer
    def nets():
        r = factory.build_renderer(wdepth=True, device="cpu", states=None)
        return [r.nerf, r.sdf_network, r.deviation_network, r.color_network, r.depth_network]
    kw = dict(factory.CONF["neus_renderer"])
    monkeypatch.delenv("VDN_PRECISION", raising=False)
    ms = nets()
    for m in (ms[0], ms[1], ms[3], ms[4]):
        del m.__dict__["precision"]          # as the runner builds them: the class default
    r = NeuSRenderer(*ms, **kw)
    assert r.precision == "fp32" and all(m.precision == "fp32" for m in (ms[0], ms[1], ms[3], ms[4]))
    r = NeuSRenderer(*nets(), precision="bf16", **kw)
    assert r.precision == "bf16" and r.sdf_network.precision == r.nerf.precision == r.color_network.precision == r.depth_network.precision == "bf16"
    monkeypatch.setenv("VDN_PRECISION", "bf16")
    r = NeuSRenderer(*nets(), **kw)
    assert r.precision == "bf16"
    r.precision = "fp32"
    assert r.sdf_network.precision == r.depth_network.precision == "fp32"
    r.sdf_network.precision = "bf16"
    assert r.precision == "mixed"
    with pytest.raises(ValueError):
        NeuSRenderer(*nets(), precision="fp16", **kw)
    with pytest.raises(ValueError):
        r.precision = "half"
    # the factory's explicit choice is not overridden by the environment default
    assert factory.build_renderer(device="cpu", precision="fp32").precision == "fp32"


def test_stream_plans_are_consistent():
    """Chunk streams: every layer's contraction width matches the previous layer's padded output."""
    s = images.sdf_streams(3, 257, 256, 8, (4,), 6)
    assert [L.kt for L in s["sdf"]] == [2, 8, 8, 8, 9, 8, 8, 8, 8]
    assert [len(L.chunks) for L in s["sdf"]] == [8, 8, 8, 7, 8, 8, 8, 8, 1]
    full = s["full"]
    assert [len(L.chunks) for L in full[9:]] == [8, 8, 8, 9, 8, 8, 8, 2]      # sweep: W7^T .. W0^T
    assert [L.kt for L in full[9:]] == [8, 8, 8, 8, 7, 8, 8, 8]
    n = images.nerf_streams(8, 256, 4, 3, 10, 4, (4,), 3, True, 96)["fwd"]
    assert [L.kt for L in n] == [3, 8, 8, 8, 8, 11, 8, 8, 8, 9, 4]
    assert [len(L.chunks) for L in n] == [8, 8, 8, 8, 8, 8, 8, 8, 9, 4, 4]
    r = images.rendering_streams(256, "idr", 9, 96, 256, 4, 4)["fwd"]
    assert [L.kt for L in r] == [10, 8, 8, 8, 8] and len(r[-1].chunks) == 3


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_chunk_tables_cover_every_chunk_once(precision):
    """The descriptor tables of vdn_build_images, built on the host (no GPU needed): every chunk of every stream gets its
    bias / pad block from exactly ONE descriptor, its k-tiles from descriptors that tile the contraction width without
    overlap, and the streams that carry a tail (row 0 of W8 in the scaled SDF streams, the normal-z column in the colour
    head's "c2" stream) carry it in every chunk."""
    rend = factory.build_renderer(wdepth=True, device="cpu", states=synth.make_all_states(2, wdepth=True), precision=precision)
    fmt = images.FMT_F32 if precision == "fp32" else images.FMT_BF16
    for net in (rend.sdf_network, rend.color_network, rend.depth_network, rend.nerf):
        im = images.NetImages(net._matrices(), net._streams(), torch.device("cpu"), fmt)
        im._build_tables()
        ch = np.frombuffer(im.chunk_table.numpy().tobytes(), dtype=lib.struct_dtype("VdnChunkDesc"))
        by_dst = {}
        for d in ch:
            by_dst.setdefault(int(d["dst"]), []).append(d)
        for dst, ds in by_dst.items():
            assert sum(int(d["write_bias"]) for d in ds) == 1, (type(net).__name__, precision)
            kt = int(ds[0]["k_pad"]) // 32
            cover = sorted((int(d["kt_begin"]), int(d["kt_count"]) or kt) for d in ds)
            assert cover[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(cover, cover[1:])) and cover[-1][0] + cover[-1][1] == kt
        if precision == "bf16" and net is rend.sdf_network:
            assert all(int(d["tail"]) != 0 and int(d["tail_n"]) == 256 and int(d["tail_stride"]) == 1 for d in ch if int(d["fmt"]) == 1 and
                       any(int(d["dst"]) >= b.data_ptr() and int(d["dst"]) < b.data_ptr() + b.numel() for k, b in im.blobs.items() if k in ("sdf", "full")))
        if precision == "bf16" and net is rend.color_network:
            c2 = im.blobs["c2"]
            mine = [d for d in ch if c2.data_ptr() <= int(d["dst"]) < c2.data_ptr() + c2.numel()]
            assert len(mine) == 33 and all(int(d["tail_stride"]) == 289 and int(d["tail_n"]) == 256 for d in mine)
            assert all(int(d["tail"]) == im.weff.data_ptr() + 4 * (im.w_off["lin0"] + 32) for d in mine)
        if precision == "fp32":
            assert "c2" not in im.blobs


def test_code_warm_up_sizes_stay_inside_their_kernels(tmp_path):
    """csrc/vdn_common.h warm_code_issue: the first workgroups of a training-step kernel read kWarmCode* bytes of their own code from
    the warm-up site on (s_getpc), so that every XCD's L2 holds it before the other workgroups arrive. Reads past the kernel's end
    would leave the loaded code object: for every kernel a `// symbol:` note names, in the library that ships, the disassembly gives
    the offset of every s_getpc_b64 inside the symbol (the compiler, not the source, decides where the site lands), and
    offset + constant must stay inside the symbol."""
    import os
    import shutil
    import subprocess
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "llvm-objdump")):
        pytest.skip("no llvm-objdump")
    from vdn_hip import build
    shutil.copy(build.LIB, tmp_path / "lib.so")
    subprocess.run([os.path.join(llvm, "llvm-objdump"), "--offloading", str(tmp_path / "lib.so")], check=True, capture_output=True)
    src = open(os.path.join(os.path.dirname(build.__file__), "..", "csrc", "vdn_common.h")).read()
    notes = re.findall(r"constexpr int (kWarmCode\w+) = (\d+) \* 1024;\s*// symbol: (\S+)", src)
    assert len(notes) >= 8
    syms = {}           # name -> (size, file, address)
    for f in sorted(os.listdir(tmp_path)):
        if "amdgcn" not in f:
            continue
        out = subprocess.run([os.path.join(llvm, "llvm-readelf"), "-s", "-W", str(tmp_path / f)], check=True, capture_output=True, text=True).stdout
        for line in out.splitlines():
            p = line.split()
            if len(p) >= 8 and p[3] == "FUNC":
                syms[p[7]] = (int(p[2], 0), f, int(p[1], 16))
    assert syms
    checked = 0
    for name, kib, sub in notes:
        match = {n: v for n, v in syms.items() if re.search(sub, n)}
        assert match, (name, sub)
        for n, (size, f, addr) in match.items():
            dis = subprocess.run([os.path.join(llvm, "llvm-objdump"), "-d", "--disassemble-symbols=" + n, str(tmp_path / f)],
                                 check=True, capture_output=True, text=True).stdout
            # the warm-up site is `s_getpc_b64 s[N:N+1]` whose low half is rounded down to 16 bytes (`s_and_b32 sN, sN, -16`) within the
            # next instructions; the compiler's own s_getpc (pc-relative addresses, relaxed long branches) add a literal instead
            lines = dis.splitlines()
            sites = []
            for i, ln in enumerate(lines):
                m = re.search(r"s_getpc_b64 s\[(\d+):\d+\]\s*//\s*([0-9A-Fa-f]+):", ln)
                if m and any(re.search(r"s_and_b32 s%s, s%s, -16\b" % (m.group(1), m.group(1)), x) for x in lines[i + 1:i + 5]):
                    sites.append(int(m.group(2), 16) - addr)
            assert sites, (name, n, "no s_getpc in the kernel: the warm-up site is gone")
            assert all(0 <= o < size for o in sites), (name, n, sites, size)
            # (+ 16: the site's address is rounded down to 16 bytes, the slices up to 256 inside `bytes & ~255`)
            assert max(sites) + int(kib) * 1024 + 16 <= size, (name, n, max(sites), kib, size)
            checked += 1
    assert checked >= 8


def test_nothing_but_the_dma_statements_writes_m0_in_the_weight_stream_kernels():
    """csrc/vdn_common.h glds16_imm*: a wave's LDS-DMA pieces of one chunk share ONE write of M0. vdn_hip.build.scan_m0_writers is the
    post-link gate that fails the build (of every variant) when anything but the DMA statements writes M0 in a kernel that issues
    LDS-DMA; here it is run on the library that ships, and must have seen the kernels."""
    import os
    from vdn_hip import build
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("no llvm-objdump")
    kernels, writes = build.scan_m0_writers(build.LIB)
    assert kernels >= 20 and writes >= 1000


def test_the_fused_sdf_kernels_of_the_product_library_use_the_32x32x16_mfma(tmp_path):
    """csrc/k_sdf_fwd2.h has one MFMA shape (the 16x16x32 arm was built for the round-6 A/B, level in wall time, never
    shipped and since removed): every sdf_fwd2_kernel instantiation of the library that ships holds v_mfma_f32_32x32x16_bf16 and no
    v_mfma_f32_16x16x32_bf16."""
    import os
    import shutil
    import subprocess
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "llvm-objdump")):
        pytest.skip("no llvm-objdump")
    from vdn_hip import build
    shutil.copy(build.LIB, tmp_path / "lib.so")
    subprocess.run([os.path.join(llvm, "llvm-objdump"), "--offloading", str(tmp_path / "lib.so")], check=True, capture_output=True)
    seen = 0
    for f in sorted(os.listdir(tmp_path)):
        if "amdgcn" not in f:
            continue
        out = subprocess.run([os.path.join(llvm, "llvm-readelf"), "-s", "-W", str(tmp_path / f)], check=True, capture_output=True, text=True).stdout
        names = sorted({p[7] for p in (line.split() for line in out.splitlines()) if len(p) >= 8 and p[3] == "FUNC" and "sdf_fwd2_kernel" in p[7]})
        for n in names:
            dis = subprocess.run([os.path.join(llvm, "llvm-objdump"), "-d", "--disassemble-symbols=" + n, str(tmp_path / f)],
                                 check=True, capture_output=True, text=True).stdout
            n16, n32 = dis.count("v_mfma_f32_16x16x32_bf16"), dis.count("v_mfma_f32_32x32x16_bf16")
            # (every program holds the eight hidden layers: 464 k-tiles of two MFMAs; the sdf-only mode's last chunk is dead code, its
            # row being the f32 dot of layer 7's epilogue)
            assert n32 >= 928 and n16 == 0, (n, n16, n32)
            seen += 1
    assert seen >= 8, seen
