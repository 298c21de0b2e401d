"""CPU: host-side logic and the C-ABI library surface (no compute calls, no GPU)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import ROOT, golden_names, load_golden

HEADER = os.path.join(ROOT, "include", "iqvit.h")


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = re.findall(r"\b(iq_[a-z0-9_]+)\s*\(", src)
    return sorted(set(names))


def test_library_loads_and_exports_every_declared_symbol():
    import vit_vs_raw_iq_amd._native as N
    assert os.path.exists(N.LIB_PATH), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(N.LIB_PATH)
    names = declared_functions()
    assert len(names) >= 35
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/iqvit.h but not exported by libiqvit.so"
    # and the ctypes binding covers exactly the header
    assert sorted(N.SIGNATURES) == names
    N.lib()


def test_struct_layouts_match_the_header_field_order():
    import vit_vs_raw_iq_amd._native as N
    src = open(HEADER).read()

    def fields(struct):
        body = re.search(r"typedef struct %s \{(.*?)\}" % struct, src, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        out = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            for part in decl.split(","):
                out.append(re.findall(r"[A-Za-z_][A-Za-z0-9_]*", part)[-1])
        return out

    assert fields("iq_dropout") == [f[0] for f in N.Dropout._fields_]
    assert fields("iq_epilogue") == [f[0] for f in N.Epilogue._fields_]
    assert fields("iq_model_cfg") == [f[0] for f in N.ModelCfg._fields_]
    assert fields("iq_wgrad_problem") == [f[0] for f in N.WgradProblem._fields_]
    assert fields("iq_reduce_seg") == [f[0] for f in N.ReduceSeg._fields_]


def test_host_only_queries_work_without_a_gpu():
    """Pure host functions of the ABI (layout / planning) are callable on CPU."""
    import vit_vs_raw_iq_amd._native as N
    L = N.lib()
    assert L.iq_ln_supported(192) == 1 and L.iq_ln_supported(20) == 0
    assert L.iq_attn_supported(197, 64) == 1 and L.iq_attn_supported(1025, 64) == 1 and L.iq_attn_supported(5000, 64) == 0
    assert L.iq_attn_supported(197, 48) == 0
    assert L.iq_wgrad_ws_bytes(50432, 768, 192) > 0
    cfg = N.ModelCfg(kind=0, in_channels=1, img_h=224, img_w=224, patch=16, seq_length=0, conv_k=0, use_cls=1,
                     num_classes=19, d_model=192, n_head=3, n_layers=12, ffn_hidden=768, drop_prob=0.1)
    h = ctypes.c_void_p()
    assert L.iq_model_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    assert L.iq_model_tokens(h) == 197
    # parameter entries cover exactly the reference's parameter count (5,391,571)
    total = 0
    name = ctypes.create_string_buffer(256)
    off, nd, dims = ctypes.c_size_t(), ctypes.c_int(), (ctypes.c_int * 4)()
    offs = []
    for i in range(L.iq_model_param_entries(h)):
        assert L.iq_model_param_entry(h, i, name, 256, ctypes.byref(off), ctypes.byref(nd), dims) == 0
        n = 1
        for k in range(nd.value):
            n *= dims[k]
        total += n
        offs.append((off.value, n))
        assert off.value % 8 == 0
    assert total == 5391571
    offs.sort()
    for (o1, n1), (o2, _) in zip(offs, offs[1:]):
        assert o1 + n1 <= o2, "parameter entries overlap"
    assert L.iq_model_param_floats(h) >= offs[-1][0] + offs[-1][1]
    # stage ranges tile the flat gradient: embedding | layers | head
    o, ln = ctypes.c_size_t(), ctypes.c_size_t()
    pos = 0
    for s in range(0, 14):
        assert L.iq_model_grad_range(h, s, s, ctypes.byref(o), ctypes.byref(ln)) == 0
        assert o.value == pos
        pos += ln.value
    assert pos == L.iq_model_param_floats(h)
    assert L.iq_model_workspace_bytes(h, 256, 1) > 256 * 197 * 192 * 2 * 12 * 8
    L.iq_model_destroy(h)
    bad = N.ModelCfg(kind=0, in_channels=1, img_h=32, img_w=32, patch=16, seq_length=0, conv_k=0, use_cls=1,
                     num_classes=3, d_model=100, n_head=4, n_layers=1, ffn_hidden=64, drop_prob=0.0)
    assert L.iq_model_create(ctypes.byref(bad), ctypes.byref(h)) != 0      # head dim 25: refused, not emulated
    # the one-launch layer tail (ffn_chain.hip): widths 128 | 192, hidden size in 64-unit chunks, ring + vectors within 160 KB
    assert L.iq_ffn_chain_supported(197, 192, 768) == 1 and L.iq_ffn_chain_supported(65, 128, 1024) == 1
    assert L.iq_ffn_chain_supported(197, 256, 1024) == 0 and L.iq_ffn_chain_supported(197, 192, 96) == 0
    assert L.iq_ffn_chain_supported(197, 192, 4096) == 0
    # rows per wave / waves per workgroup by row count: 32 x 7 above 32,768 rows, 16 x 8 down to 20,481, 16 x 5 below
    for M, rw, nw in ((50432, 32, 7), (33024, 32, 7), (32768, 16, 8), (25216, 16, 8), (20480, 16, 5), (16640, 16, 5), (153, 16, 5)):
        units = (M + rw - 1) // rw
        assert L.iq_ffn_chain_bwd_partial_rows(M) == (units + nw - 1) // nw, M
        assert L.iq_ffn_chain_gate_bytes(M, 768) == units * 12 * 256, M
    # the fused data-gradient GEMM + LayerNorm backward: 64-row blocks up to 320 blocks of 128 rows, 128-row blocks above
    assert L.iq_gemm_lnbwd_partial_rows(40960) == 640 and L.iq_gemm_lnbwd_partial_rows(40961) == 321


@pytest.mark.parametrize("name", golden_names())
def test_module_surface_matches_reference_state_dict(name):
    """Constructor kwargs, state_dict keys/shapes and seeded initial values (CPU construction only)."""
    import numpy as np
    import vit_vs_raw_iq_amd as P
    import iq_oracle as O
    kind, kw, z = load_golden(name)
    torch.manual_seed(int(z["seed"]))
    m = (P.AMCTransformerViT if kind == "vit" else P.AMCTransformerRawIQ)(drop_prob=0.0, device="cpu", **kw)
    sd = O.init_state(O.OracleConfig(kind=kind, drop_prob=0.0, **kw), int(z["seed"]))
    got = m.state_dict()
    assert list(sorted(got)) == list(sorted(sd))
    for k in sd:
        assert torch.equal(got[k], sd[k]), k
    assert np.array_equal(got["encoder.positional_encoding.encoding"].numpy(), z["pe"])
    assert sum(p.numel() for p in m.parameters()) == int(z["n_params"])


def test_reference_import_paths_and_error_conventions():
    from vit_vs_raw_iq_amd.ViT.models.amc_transformer import AMCTransformer as V
    from vit_vs_raw_iq_amd.transformer_rawIQ.models.transformer_rawIQ import AMCTransformer as R
    import vit_vs_raw_iq_amd as P
    assert V is P.AMCTransformerViT and R is P.AMCTransformerRawIQ
    # hyperparameter_tuning.py:22-34 / :41-54 call surfaces
    V(in_channels=1, img_size_h=32, img_size_w=32, patch_size=16, num_classes=11, d_model=128, n_head=8, n_layers=1,
      ffn_hidden=256, drop_prob=0.1, device="cpu")
    r = R(in_channels=2, seq_length=1024, num_classes=11, d_model=128, n_head=8, n_layers=1, ffn_hidden=256,
          drop_prob=0.1, device="cpu", use_cls_token=True, embedding_type="segment", segment_size=64)
    with pytest.raises(ValueError, match=r"seq_length \(1000\) must be divisible by segment_size \(64\)"):
        R(in_channels=2, seq_length=1000, num_classes=3, d_model=64, n_head=4, n_layers=1, ffn_hidden=64,
          drop_prob=0.0, device="cpu", segment_size=64)
    with pytest.raises(ValueError, match="Unknown embedding_type: patch"):
        R(in_channels=2, seq_length=1024, num_classes=3, d_model=64, n_head=4, n_layers=1, ffn_hidden=64,
          drop_prob=0.0, device="cpu", embedding_type="patch")
    with pytest.raises(ValueError, match="segment_size is required"):
        P.SequenceEmbedding(method="segment")
    with pytest.raises(ValueError, match="Unknown method"):
        P.SequenceEmbedding(method="foo")
    # the product path never computes on CPU
    with pytest.raises(P.IqError, match="no CPU fallback"):
        r(torch.zeros(1, 2, 1024))


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "vit-vs-raw-iq_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "iq_oracle" not in text and "import oracle" not in text, os.path.join(dirpath, f)
    code = ("import sys; sys.path.insert(0, %r); import vit_vs_raw_iq_amd, vit_vs_raw_iq_amd.trainer; "
            "assert 'iq_oracle' not in sys.modules" % ROOT)
    subprocess.check_call([sys.executable, "-c", code])


def test_bucket_plan_covers_every_stage_once():
    from vit_vs_raw_iq_amd.trainer import make_buckets
    for L_ in (0, 1, 2, 6, 12):
        for nb in (1, 2, 3, 4, 7, 50):
            b = make_buckets(L_, nb)
            stages = []
            for hi, lo in b:
                assert hi >= lo
                stages += list(range(hi, lo - 1, -1))
            assert stages == list(range(L_ + 1, -1, -1))


def test_counted_tail_waits_match_the_isa():
    """The GEMM kernels wait for their last operand stage with `s_waitcnt vmcnt(N)`, N = the tail loads issued behind it.
    That is only correct if the compiler emitted at least N loads there: checked in the gfx950 ISA (hipcc cross-compiles)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "dbg", "check_epi_counts.py")], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "ok:" in r.stdout


def test_pingpong_kernels_hold_their_state_in_registers():
    """gemm_big / wgrad_big / the gemm_ln band kernel count their DMA queue by hand: a spilled register is a scratch
    reload, i.e. a vmcnt entry the counts do not know (it drained the queue and cost 30 % when it happened) -- the gfx950
    ISA of those kernels must show no spill and no scratch, and one workgroup's worth of registers (<= 256)."""
    import re
    import tempfile
    csrc = os.path.join(ROOT, "vit-vs-raw-iq_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    seen = 0
    for src, pat in (("gemm_big.hip", "gemm_big_kernel"), ("gemm_wgrad_big.hip", "wgrad_big_kernel"), ("gemm_ln.hip", "gemm_ln_band_kernel")):
        out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
                               "-S", "--cuda-device-only", os.path.join(csrc, src), "-o", out], stderr=subprocess.DEVNULL)
        text = open(out).read()
        os.unlink(out)
        for m in re.finditer(r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text, re.S):
            name, scratch, vgpr, spill = m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4))
            if pat in name:
                seen += 1
                assert scratch == 0 and spill == 0 and vgpr <= 256, (name, scratch, vgpr, spill)
    assert seen == 3 + 3 + 1


def test_chain_kernels_keep_scratch_out_of_their_chunk_loops_and_pad_their_inline_asm():
    """The one-launch layer kernels (ffn_chain.hip) stream their weights through an LDS ring behind COUNTED `s_waitcnt vmcnt(N)`:
    a register reloaded from scratch inside a chunk loop is a vector-memory load the counts do not know, and the compiler waits
    `vmcnt(0)` for it -- the ring drains every iteration (it happened twice while these kernels were written; spills OUTSIDE
    the loops, in the one-off tails, are harmless).  Checked in the gfx950 ISA: no scratch access in any loop that issues MFMAs."""
    import re
    import tempfile
    csrc = os.path.join(ROOT, "vit-vs-raw-iq_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
                           "-S", "--cuda-device-only", os.path.join(csrc, "ffn_chain.hip"), "-o", out], stderr=subprocess.DEVNULL)
    text = open(out).read()
    os.unlink(out)
    # Inline-asm memory instructions that take their base address in scalar registers start with `s_nop 4`: the compiler restores a
    # spilled scalar with v_readlane_b32 right in front of the asm, and a vector-memory instruction reading an SGPR written by a
    # VALU instruction needs five wait states the hazard recogniser does not insert in front of inline asm (two GPU faults).
    alines = text.split("\n")
    nasm = 0
    for i, ln in enumerate(alines):
        if "ASMSTART" in ln:
            blk = []
            j = i + 1
            while "ASMEND" not in alines[j]:
                blk.append(alines[j].strip()); j += 1
            if any(re.search(r"^global_\S+.*\bs\[\d+:\d+\]", x) for x in blk):
                nasm += 1
                assert blk[0] == "s_nop 4", blk
    assert nasm > 100, nasm
    kernels = loops = 0
    for fn in re.split(r"\n(?=_ZN\S*ffn_chain_(?:fwd|bwd)_kernel\S*:)", text)[1:]:
        name = fn.split(":", 1)[0]
        lines = re.split(r"\n\.Lfunc_end\d+:", fn, 1)[0].split("\n")      # (a kernel may hold several s_endpgm)
        # basic blocks and their edges; a loop = a strongly connected component of the control-flow graph (block layout in the
        # text says nothing: the compiler moves loop latches out of line)
        blocks, cur = [], {"label": None, "ins": [], "succ": [], "fall": True}
        for ln in lines[1:]:
            m = re.match(r"^(\.LBB\d+_\d+):", ln)
            if m:
                blocks.append(cur)
                cur = {"label": m.group(1), "ins": [], "succ": [], "fall": True}
                continue
            if not re.match(r"^\s+[a-z]", ln):
                continue
            op = ln.split()[0]
            cur["ins"].append(op)
            t = re.match(r"^\s+s_c?branch\S*\s+(\.LBB\d+_\d+)", ln)
            if t:
                cur["succ"].append(t.group(1))
            if op in ("s_branch", "s_endpgm", "s_setpc_b64") or t:
                cur["fall"] = op not in ("s_branch", "s_endpgm", "s_setpc_b64")
                blocks.append(cur)
                cur = {"label": None, "ins": [], "succ": [], "fall": True}
        blocks.append(cur)
        index = {b["label"]: i for i, b in enumerate(blocks) if b["label"]}
        edges = [[index[t] for t in b["succ"] if t in index] + ([i + 1] if b["fall"] and i + 1 < len(blocks) else [])
                 for i, b in enumerate(blocks)]
        # Tarjan, iterative
        n = len(blocks)
        idx, low, on, st, comps, counter = [-1] * n, [0] * n, [False] * n, [], [], 0
        for root in range(n):
            if idx[root] != -1:
                continue
            work = [(root, 0)]
            while work:
                v, ei = work.pop()
                if ei == 0:
                    idx[v] = low[v] = counter; counter += 1; st.append(v); on[v] = True
                recurse = False
                for k in range(ei, len(edges[v])):
                    w = edges[v][k]
                    if idx[w] == -1:
                        work.append((v, k + 1)); work.append((w, 0)); recurse = True
                        break
                    if on[w]:
                        low[v] = min(low[v], idx[w])
                if recurse:
                    continue
                if low[v] == idx[v]:
                    comp = []
                    while True:
                        w = st.pop(); on[w] = False; comp.append(w)
                        if w == v:
                            break
                    comps.append(comp)
                if work:
                    u = work[-1][0]
                    low[u] = min(low[u], low[v])
        kernels += 1
        found = 0
        for comp in comps:
            if len(comp) == 1 and comp[0] not in edges[comp[0]]:
                continue
            body = [op for bi in comp for op in blocks[bi]["ins"]]
            if any(x.startswith("v_mfma") for x in body):
                found += 1
                assert not any(x.startswith("scratch_") for x in body), f"{name}: scratch access inside an MFMA loop"
        assert found >= 1, f"{name}: no MFMA loop found"
        loops += found
    assert kernels == 72 and loops >= kernels, (kernels, loops)      # 2 widths x 3 shapes x 2 dropout x 3 stage modes, fwd + bwd


def test_bench_dump_outputs_keeps_its_budget_and_samples_the_same_elements(tmp_path, monkeypatch):
    """bench.py --dump-outputs: small arrays are written whole; large ones, when they would pass the byte budget, as one
    seeded sample of their elements -- the same one in every run, so two builds compare element for element."""
    import numpy as np
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 64 << 10)
    monkeypatch.setattr(bench, "DUMP_WHOLE", 1000)
    rng = np.random.default_rng(3)
    arrays = {"logits": rng.standard_normal((16, 19), dtype=np.float32), "params": rng.standard_normal(40000, dtype=np.float32),
              "grads": rng.standard_normal(40000, dtype=np.float32), "final_loss": np.array([2.5])}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    total = 0
    for name, v in arrays.items():
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == v.dtype and np.array_equal(a, b)
        total += os.path.getsize(tmp_path / "a" / f"{name}.npy")
        if v.size <= 1000:
            assert np.array_equal(a, v)
        else:
            assert 0 < a.size < v.size and np.isin(a, v).all()
    assert total <= 64 << 10
    bench.dump_outputs(str(tmp_path / "c"), {"params": arrays["params"][:10000]})       # fits: written whole
    assert np.array_equal(np.load(tmp_path / "c" / "params.npy"), arrays["params"][:10000])
