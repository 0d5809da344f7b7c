"""CPU: host-side surface that mirrors the reference (flags, module tree, checkpoint keys, meters,
synthetic data contract).  No kernels are launched."""
import numpy as np
import pytest
import torch

from mclstexp_amd import synth


def test_generate_args_keeps_reference_flags_and_defaults():
    """train.py:11-27: the 13 flags, names/defaults unchanged."""
    from mclstexp_amd.train import generate_args
    a = generate_args([])
    ref = dict(batch_size=128, max_epochs=90, temperature=1.0, fold=0, dim=785, image_embedding_dim=1024,
               projection_dim=256, heads_num=8, heads_dim=64, heads_layers=2, dropout=0.0, dataset="her2st",
               encoder_name="densenet121")
    for k, v in ref.items():
        assert getattr(a, k) == v, k
    b = generate_args(["--batch_size", "8", "--dim", "1000", "--encoder_name", "vit", "--image_embedding_dim", "768"])
    assert (b.batch_size, b.dim, b.encoder_name, b.image_embedding_dim) == (8, 1000, "vit", 768)


def test_state_dict_keys_match_reference_layout():
    """SURVEY Appendix A.3 keys (captured from the imported reference)."""
    from mclstexp_amd.model import mclSTExp_Attention
    m = mclSTExp_Attention("densenet121", 1.0, 1024, 171, 256, 8, 64, 2)
    keys = set(m.state_dict())
    want = set(synth.param_spec(171, 1024))
    assert want <= keys
    assert "image_encoder.model.0.denseblock1.denselayer1.conv1.weight" in keys
    assert "image_encoder.model.0.norm5.running_mean" in keys
    assert "image_encoder.model.0.transition3.conv.weight" in keys
    non_backbone = {k for k in keys if not k.startswith("image_encoder.")}
    assert non_backbone == want
    for attr in ("image_encoder", "image_projection", "x_embed", "y_embed", "spot_encoder", "spot_projection",
                 "temperature"):
        assert hasattr(m, attr)                 # evel_her2st.py:48-69 uses these directly
    assert m.x_embed.weight.shape == (65536, 171)
    n = sum(p.numel() for p in m.image_encoder.parameters())
    assert n == 6953856                          # torchvision densenet121.features parameter count


def test_unknown_encoder_raises_and_mlp_attr_name():
    from mclstexp_amd.model import mclSTExp_Attention, mclSTExp_MLP
    with pytest.raises(ValueError):
        mclSTExp_Attention("nope", 1.0, 1024, 171, 256, 8, 64, 2)
    m = mclSTExp_MLP(1.0, 1024, 171, 256, encoder_name="identity")
    assert hasattr(m, "image_ecode")             # model.py:176 (sic)


def test_checkpoint_key_rewrites():
    """evel_her2st.py:33-37: strip 'module.', rename 'well' -> 'spot'."""
    from mclstexp_amd.model import load_reference_state_dict, mclSTExp_Attention
    m = mclSTExp_Attention("identity", 1.0, 1024, 171, 256, 8, 64, 1)
    sd = {("module." + k).replace("spot", "well"): v.clone() + 1 for k, v in m.state_dict().items()}
    load_reference_state_dict(m, sd)
    assert torch.equal(m.state_dict()["spot_projection.fc.bias"], sd["module.well_projection.fc.bias"])


def test_avgmeter_and_get_lr():
    from mclstexp_amd.utils import AvgMeter, get_lr
    a = AvgMeter()
    a.update(2.0, 128); a.update(4.0, 64)
    assert abs(a.avg - (2 * 128 + 4 * 64) / 192) < 1e-12 and "Metric" in repr(a)
    p = torch.nn.Parameter(torch.zeros(1))
    assert get_lr(torch.optim.Adam([p], lr=1e-4)) == 1e-4


def test_synth_is_deterministic_and_row_addressable():
    full = synth.uniform_tensor("x_embed.weight", (65536, 7), -1, 1, seed=0)
    rows = synth.uniform_tensor("x_embed.weight", (65536, 7), -1, 1, seed=0, rows=np.array([0, 5, 60000]))
    assert torch.equal(rows, full[[0, 5, 60000]])
    b = synth.make_batch(8, 785, image_dim=1024, seed=0)
    assert b["expression"].shape == (8, 785) and b["position"].shape == (8, 2) and b["image"].shape == (8, 1024)
    assert float((b["expression"] == 0).float().mean()) > 0.6
    assert torch.equal(b["position"], torch.floor(b["position"])) and b["position"].max() < 64
    assert torch.equal(synth.make_batch(8, 785, image_dim=1024, seed=0)["expression"], b["expression"])


def test_vit_and_resnet_shapes_cpu():
    from mclstexp_amd.backbones import ImageEncdoer_res18, ImageEncoder_VIT
    x = torch.rand(2, 3, 224, 224)
    with torch.no_grad():
        assert ImageEncoder_VIT().eval()(x).shape == (2, 768)       # model.py:104-116, patch32
        assert ImageEncdoer_res18().eval()(x[:, :, :64, :64]).shape == (2, 512)


def test_kernel_audit_classifies_library_kernels():
    """mclstexp_amd.kernel_audit.foreign(): library kernels (hipBLASLt / Tensile, ATen, MIOpen, rocPRIM) are flagged, this
    library's kernels and the runtime's copy / fill helpers are not."""
    from mclstexp_amd import kernel_audit
    names = ["Cijk_Ailk_Bljk_BBS_BH_Bias_HA_S_SAV_UserArgs_MT256x224x32",
             "void at::native::vectorized_elementwise_kernel<4, at::native::FillFunctor<float>, std::array<char*, 1ul> >(int)",
             "void at::native::(anonymous namespace)::multi_tensor_apply_kernel<...>", "miopenSp3AsmConv_v30_3_1_gfx9_fp32",
             "void rocprim::detail::sort_kernel<...>",
             "(anonymous namespace)::conv1x1_fwd_kernel<2, 32, 4>(unsigned short const*, long long)",
             "(anonymous namespace)::fill_zero_kernel(unsigned int*, long long)", "__amd_rocclr_copyBuffer", "Memcpy DtoD (Device -> Device)",
             "void (anonymous namespace)::gemm_bf16_kernel<false, true, 2>((anonymous namespace)::GemmB)"]
    bad = kernel_audit.foreign(names)
    assert len(bad) == 5 and all(("conv1x1" not in n and "fill_zero" not in n and "rocclr" not in n and "gemm_bf16" not in n)
                                 for n in bad)


def test_train_flags_include_fp8_infonce():
    from mclstexp_amd.train import generate_args
    a = generate_args(["--infonce", "fp8"])
    assert a.infonce == "fp8" and a.encoder_name == "densenet121" and a.dim == 785     # reference defaults untouched


def test_retrieval_filter_plan_keeps_the_expected_list_inside_its_capacity():
    """mclstexp_amd.retrieval._filter_plan (host arithmetic only): for every key count the expected candidate-list length
    stays well inside the capacity and above k -- the r05 plan overflowed for N > ~262k."""
    from mclstexp_amd import retrieval as rt
    for n in (8192, 20000, 65536, 262144, 300000, 1_000_000, 10_000_000):
        for k in (1, 50, 200, 600, 1024):
            if 16 * k > n:
                continue
            ns, step, r, cap = rt._filter_plan(n, k)
            assert ns <= n and step >= 1 and ns * step <= n and step <= rt.FUSED_MAX_STRIDE
            expect = r * n / ns
            assert expect >= 1.4 * k, (n, k)
            assert expect * (1 + 4 / r ** 0.5) < cap, (n, k, expect, cap)      # four standard deviations of the count


def test_dense_backward_layer_plan_at_the_benchmark_shapes(monkeypatch):
    """densenet_fused._plan_layer, the one decision table of DenseBlockFn.backward (booleans and integers only), walked in
    backward order over the four DenseNet-121 blocks at bench.py's default workload, the way the backward walks them (the only
    state it carries between layers: single-pass mean terms pending, a layer A waiting for its pair)."""
    import sys

    import bench
    from mclstexp_amd import densenet_fused as dn
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    args = bench.parse()
    assert (args.batch, args.image) == (128, 224)
    growth = 32
    blocks = [(6, 64, args.image // 4), (12, 128, args.image // 8), (24, 256, args.image // 16), (16, 512, args.image // 32)]

    def walk(L, C0, hw, B, own=True, side=True):
        """[(l, plan, role)] of one block; role of a Gram layer: "A" / "B" of a pair or "alone"."""
        out, kacc, pending = [], False, False
        for l in range(L - 1, -1, -1):
            p = dn._plan_layer(l, C0 + l * growth, growth, B, hw, hw, own, own, own, own, kacc, side,
                               dn.USE_BN1_SINGLE_PASS, dn.BN1_SINGLE_PASS_MAX_MAP, dn.FUSED_BN1_WRW_MIN_PIXELS)
            role = None
            if p.conv1 == "gram":
                role = "B" if pending else ("A" if p.opens_pair else "alone")
                pending = role == "A"
            else:
                pending = False                                 # (the executor flushes a waiting layer A here)
            kacc = p.conv1 == "single" or (kacc and p.fix != "launch_all")
            out.append((l, p, role))
        return out

    for side in (True, False):
        for L, C0, hw in blocks[:2]:                            # 56 x 56, 28 x 28: Gram path, dx passes in pairs
            steps = walk(L, C0, hw, args.batch, side=side)
            assert all(p.conv2 == "own" and p.conv1 == "gram" and p.fix == "none" and p.lanes == side for _, p, _ in steps)
            assert all(p.opens_pair == (l >= 1) for l, p, _ in steps)       # layer 0 never opens a pair: alone unless it closes one
            assert [r for _, _, r in steps] == ["A", "B"] * (L // 2)         # (L - 1, L - 2), ..., (1, 0)
        L, C0, hw = blocks[2]                                   # 14 x 14: single pass, correction folded from the second layer on
        steps = walk(L, C0, hw, args.batch, side=side)
        assert all(p.conv2 == "own" and p.conv1 == "single" and p.lanes == side and not p.opens_pair for _, p, _ in steps)
        assert [p.fix for _, p, _ in steps] == ["none"] + ["fold"] * (L - 1)
        L, C0, hw = blocks[0]                                   # B = 4: below the Gram threshold, map too large for the single pass
        steps = walk(L, C0, hw, 4, side=side)
        assert all(p.conv1 == "two_pass" and p.fix == "none" and p.conv2 == "own" and p.lanes == side for _, p, _ in steps)
        for L, C0, hw in blocks:                                # fp32 activations: nothing fused, nothing leaves the main chain
            for B in (4, args.batch):
                steps = walk(L, C0, hw, B, own=False, side=side)
                assert all(p == dn._LayerPlan("generic", "generic", "none", False, False) for _, p, _ in steps)
    # lanes is false whenever USE_SIDE_STREAM is false, whatever else holds
    import itertools
    for f1, f2, d1, d2, k, hw, B in itertools.product((False, True), (False, True), (False, True), (False, True), (False, True),
                                                       (7, 14, 28, 56), (4, 128)):
        p = dn._plan_layer(3, 160, growth, B, hw, hw, f1, f2, d1, d2, k, False, True, 256, 50000)
        assert p.lanes is False
        q = dn._plan_layer(3, 160, growth, B, hw, hw, f1, f2, d1, d2, k, True, True, 256, 50000)
        assert q.lanes == (f1 and f2 and d2) and q[:3] == p[:3]      # the schedule changes nothing else
        assert (p.fix == "none") == (not k) and (p.fix == "fold") <= (p.conv1 == "single" and p.conv2 == "own" and hw < 17)
        assert (p.fix == "launch_all") == (k and p.conv1 != "single")
