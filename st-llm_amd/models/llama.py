"""Vicuna-7B / Llama-1 decoder PREFILL on the HIP C ABI, HF parameter names.

The reference imports HF ``transformers.models.llama`` (st_llm.py:20; pinned 4.28.0) — third-party code
that is not in the reference tree; its in-tree statement is stllm/models/modeling_llama_mem.py:61-144.
Per layer:

    RMSNorm -> [fused QKV GEMM + rotate-half RoPE epilogue] -> causal flash attention (+ right-pad mask)
    -> [o_proj GEMM + fp32 residual] -> RMSNorm -> [gate/up GEMM + SiLU(gate)*up epilogue]
    -> [down_proj GEMM + fp32 residual]

then the final RMSNorm and lm_head on ALL positions (st_llm.py:122).  That sequence is written ONCE, in decoder_layer(); prefill, extend (plain and behind a
shared base), the sequence-parallel halves and decode_step (16-bit, int8, int4, LoRA) call it with their own projection, QKV destination and attention.

Decode with a KV cache (the step after the prefill in Chat.answer -> generate): the fused QKV
buffer of every layer IS the cache — ``KVCache`` owns one [B, max_len, 3*D] buffer per layer; the prefill GEMM writes rows
[0, S) of it through the 2-level row indexing, a decode step writes row `len` (RoPE at that position) and attends over
rows [0, len] in place: no copies, no re-layout.  Decode reuses the prefill kernels (small-M tiles); GEMV-regime kernels
are future work.

Int8 decode weights (runtime.set_decode_weights("int8")): decode_step streams an int8 copy of the four packed projection weights of every
layer (pack.quant8_rows: one fp32 scale per output row) through the W8A16 kernels (hip.gemv_w8 behind decoder_layer's projection) — half the bytes per token.  The copy lives
NEXT TO the 16-bit weights, which prefill / extend keep using: + 6.6 GB at 7B on top of the 13.5 GB of the 16-bit pack.  This is the
reference's `device_8bit` knob (demo.py:41) with something behind it.

Int4 decode weights (runtime.set_decode_weights("int4g128")): the same routing over a 4-bit copy (pack.quant4_groups: two weights per byte, one fp32 scale
per output row and group of 128 K elements) on the W4A16 kernels (hip.gemv_q4) — about 0.27 of the 16-bit bytes per token, + 3.5 GB at 7B.  One quantised
copy exists at a time (one slot, LlamaModel._quant): switching between "int8", "int4g128" and None frees the other at the next decode_step.
"""
import collections
import os

import torch
import torch.nn as nn

from .. import hip, pack, runtime
from . import lora as lora_mod
from .layers import Embedding, Linear, Output, ParamList, RMSNorm, params_fingerprint


def _frag(pk, key):
    """keyword of hip.gemm for the fragment-major copy of pk[key], when the pack made one (pack.frag32_or_none)"""
    f = pk.get(key + "_frag")
    return {"w_frag": f} if f is not None else {}


def gemm_proj(layers, dt, frag):
    """decoder_layer's `proj` on the 16-bit packed weights: hip.gemm, with the fragment-major copy where the pack made one (prefill / extend: frag=True)"""
    if frag:
        return lambda li, key, a, **kw: hip.gemm(a, layers[li][key], dtype=dt, **kw, **_frag(layers[li], key))
    return lambda li, key, a, **kw: hip.gemm(a, layers[li][key], dtype=dt, **kw)


def decoder_layer(m, dt, x, pk, li, *, proj, qkv_to, attn, rope, rope_seq, fuse=False, part=None, qkv=None):
    """THE decoder layer, on the fp32 residual x [M, D] in place:

        norm 1 -> QKV projection + RoPE -> attention -> o_proj + residual -> norm 2 -> gate/up + SwiGLU -> down + residual

    Every host path runs this body; they differ in three things only, which they pass in:
      * the operand of the QKV projection: RMSNorm(x), with active adapters (`"lora_A" in pk`) m.qkv_operand's K-extended rows, or (fuse) no operand at
        all — the norm rides inside the projection (a_norm=).  Norm 2 follows `fuse` as well; adapters never fuse norm 1.
      * proj(li, key, a, **kw): the projection of a by layer li's weight `key` (hip.gemm / hip.gemv_w8 / hip.gemv_q4 behind it, looked up on `hip` when
        called), and qkv_to(li): the keywords that say where the fused [q | k | v] rows land (none: a fresh tensor) — proj returns that destination;
      * attn(li, qkv) -> the attention output rows that o_proj consumes.
    m: the model, or a stand-in with `config` (and `qkv_operand` when adapters are active).  rope = (cos, sin) rows, row r of the projection at table
    row r % rope_seq.  part: None = the whole layer; 0 = up to and including the QKV rows (returns their destination); 1 = from the attention on, over
    `qkv` — the two halves sequence-parallel prefill interleaves its transfers with."""
    eps, D = m.config.rms_norm_eps, m.config.hidden_size
    if part != 1:
        if "lora_A" in pk:
            h, kw = m.qkv_operand(x, pk, dt), {}
        else:
            h, kw = (None, {"a_norm": (x, pk["ln1"], eps)}) if fuse else (hip.rmsnorm(x, pk["ln1"], eps, dtype=dt)[0], {})
        qkv = proj(li, "wqkv", h, epilogue=hip.EPI_ROPE, rope=rope, rope_seq=rope_seq, rope_cols=2 * D, **kw, **qkv_to(li))
        if part == 0:
            return qkv
    a = attn(li, qkv)
    proj(li, "wo", a, epilogue=hip.EPI_RESID, resid=x)
    h, kw = (None, {"a_norm": (x, pk["ln2"], eps)}) if fuse else (hip.rmsnorm(x, pk["ln2"], eps, dtype=dt)[0], {})
    g = proj(li, "wgu", h, epilogue=hip.EPI_SWIGLU, **kw)
    proj(li, "wdown", g, epilogue=hip.EPI_RESID, resid=x)


class LlamaConfig:
    model_type = "llama"

    def __init__(self, hidden_size=4096, intermediate_size=11008, num_hidden_layers=32, num_attention_heads=32,
                 vocab_size=32000, rms_norm_eps=1e-6, max_position_embeddings=2048, rope_theta=10000.0, **kw):
        self.hidden_size, self.intermediate_size = hidden_size, intermediate_size
        self.num_hidden_layers, self.num_attention_heads = num_hidden_layers, num_attention_heads
        self.vocab_size, self.rms_norm_eps = vocab_size, rms_norm_eps
        self.max_position_embeddings, self.rope_theta = max_position_embeddings, rope_theta
        self.__dict__.update(kw)


class LlamaAttention(nn.Module):
    def __init__(self, cfg, device):
        super().__init__()
        d = cfg.hidden_size
        self.q_proj = Linear(d, d, bias=False, device=device)
        self.k_proj = Linear(d, d, bias=False, device=device)
        self.v_proj = Linear(d, d, bias=False, device=device)
        self.o_proj = Linear(d, d, bias=False, device=device)


class LlamaMLP(nn.Module):
    def __init__(self, cfg, device):
        super().__init__()
        self.gate_proj = Linear(cfg.hidden_size, cfg.intermediate_size, bias=False, device=device)
        self.up_proj = Linear(cfg.hidden_size, cfg.intermediate_size, bias=False, device=device)
        self.down_proj = Linear(cfg.intermediate_size, cfg.hidden_size, bias=False, device=device)


class LlamaDecoderLayer(nn.Module):
    def __init__(self, cfg, device):
        super().__init__()
        self.self_attn = LlamaAttention(cfg, device)
        self.mlp = LlamaMLP(cfg, device)
        self.input_layernorm = RMSNorm(cfg.hidden_size, cfg.rms_norm_eps, device)
        self.post_attention_layernorm = RMSNorm(cfg.hidden_size, cfg.rms_norm_eps, device)

    def pack(self, dt, n_heads, frag=True, lora=True):
        a, m = self.self_attn, self.mlp
        pk = dict(ln1=self.input_layernorm.weight, ln2=self.post_attention_layernorm.weight,
                  wqkv=pack.llama_qkv(a.q_proj.weight, a.k_proj.weight, a.v_proj.weight, dt, n_heads),
                  wo=pack.linear(a.o_proj.weight, dt),
                  wgu=pack.llama_gate_up(m.gate_proj.weight, m.up_proj.weight, dt),
                  wdown=pack.linear(m.down_proj.weight, dt))
        # fragment-major copy of wqkv for the W-direct prefill GEMM (csrc/gemm_wd.inc, round 6): + 100 MB per layer (3.2 GB at 7B in 16 bits).  The gate/up
        # weight gets none: its 86 column blocks never make the one-round plans the dispatcher takes (measured equal or slower, profiles/r06_bench_ab_wd.log);
        # the C entry point and hip.gemm accept one all the same (stllm_llama_layer_weights.wgu_frag, w_frag=)
        pk["wqkv_frag"] = pack.frag32_or_none(pk["wqkv"]) if (frag and dt != torch.float32) else None   # (fp32 / bf16x3: other kernels)
        pk["wgu_frag"] = None
        ad = lora_mod.adapters_of(self) if lora else None
        if ad is not None:
            # active LoRA adapters: the QKV weight gets P extra K columns holding s B (models/lora.py: extend_qkv) and the prefill / decode GEMM runs over
            # K = hidden + P.  The W-direct kernel needs K % 256 == 0: no fragment-major copy, the dispatcher takes the 128 x 256 one-wave tile instead
            if runtime.gemm_split():
                raise NotImplementedError("LoRA adapters in the bf16x3 / mixed modes: merge_adapter() first (the split GEMMs have no K-extended path)")
            pk["wqkv"], pk["lora_A"], pk["lora_r"], pk["lora_P"] = lora_mod.extend_qkv(pk["wqkv"], ad[0], ad[1], dt, n_heads)
            pk["wqkv_frag"] = None
        return pk


def cfg_max_len(cfg):
    return int(getattr(cfg, "max_position_embeddings", 2048))


class KVCache:
    """Per-layer fused [q | k | v] rows (compute dtype, k/q in the packed RoPE head layout).
    `lens` is None for a UNIFORM cache — every row holds `len` positions (a clip, or the beams of one clip): the only kind there was, and its code paths
    are untouched.  Otherwise the cache is RAGGED: `lens` is a host list of `batch` ints, row b holds positions [0, lens[b]) and `len` == max(lens), so
    bounds checks against `len` keep their meaning.  prefill() with a right-padded mask and extend(lengths=) make a cache ragged; decode_step then appends
    token b at position lens[b] (RoPE at that position) and row b attends its own lens[b] + 1 keys.  Rows behind lens[b] hold don't-care
    values that later steps overwrite.
    `base` is None for the cache described so far.  share() makes a cache with a BASE: the first base_len = P positions of every row live
    in another cache, held by reference and never written — row b reads base row b // (batch // base.batch), so the rows come in contiguous groups that
    share one physical prefix — and `qkv` holds the positions >= P only, [batch, max_len - P, 3 * hidden], local index = position - P.  `len`, `lens` and
    `max_len` keep counting TOTAL positions (RoPE positions, bounds checks).  One level only: the base has no base."""

    def __init__(self, n_layers, batch, max_len, hidden, dtype, device, base=None):
        self.max_len, self.batch, self.hidden = max_len, batch, hidden
        self.base, self.base_len = base, (base.len if base is not None else 0)
        self.qkv = [torch.empty((batch, max_len - self.base_len, 3 * hidden), device=device, dtype=dtype) for _ in range(n_layers)]
        self.len = self.base_len
        self.lens = None

    def flat(self, li):
        """layer li's own buffer as 2-D rows [batch * capacity, 3 * hidden]: row (b, local position s) at b * capacity + s"""
        buf = self.qkv[li]
        return buf.view(buf.shape[0] * buf.shape[1], buf.shape[2])

    def kv(self, li):
        """(k, v, strides): the K and V columns of flat(li) and their (batch stride, row stride) in elements — what the attention entry points take"""
        D, rows = self.hidden, self.flat(li)
        return rows[:, D:2 * D], rows[:, 2 * D:], (self.qkv[li].shape[1] * 3 * D, 3 * D)

    def set_lens(self, lens):
        """per-row lengths (a list of `batch` ints) -> ragged; None, or all rows equal -> uniform"""
        if lens is None or len(set(lens)) <= 1:
            if lens is not None:
                self.len = int(lens[0])
            self.lens = None
            return
        lens = [int(n) for n in lens]
        assert len(lens) == self.batch and min(lens) >= 0 and max(lens) <= self.max_len
        self.lens, self.len = lens, max(lens)

    def fork(self, rows=None, max_len=None):
        """a new cache holding copies of the first `len` positions, every source row repeated rows // batch times (the beams of a prompt; a
        reusable prefix that generation must not write behind).  max_len defaults to this cache's."""
        rows = self.batch if rows is None else rows
        max_len = self.max_len if max_len is None else max_len
        assert rows % self.batch == 0 and max_len >= self.len
        new = KVCache(len(self.qkv), rows, max_len, self.hidden, self.qkv[0].dtype, self.qkv[0].device)
        n, rep = self.len, rows // self.batch
        if self.base is not None:   # a cache with a base materialises: a dense private copy of base rows + suffix rows (for paths that do not share)
            P, grp = self.base_len, rows // self.base.batch
            for dst, pre, src in zip(new.qkv, self.base.qkv, self.qkv):
                dst[:, :P] = pre[:, :P].repeat_interleave(grp, dim=0) if grp > 1 else pre[:, :P]
                dst[:, P:n] = src[:, :n - P].repeat_interleave(rep, dim=0) if rep > 1 else src[:, :n - P]
        else:
            for dst, src in zip(new.qkv, self.qkv):
                dst[:, :n] = src[:, :n].repeat_interleave(rep, dim=0) if rep > 1 else src[:, :n]
        new.len = n
        if self.lens is not None:   # ragged: every copy of a row inherits its length
            new.lens = [l for l in self.lens for _ in range(rep)]
        return new

    def share(self, rows=None, max_new=None):
        """a new cache whose first positions are THIS cache, by reference: nothing is copied, this cache is never written through it, and the decode
        attention reads its K / V once per group of rows instead of once per row (hip.attention_shared).  Every row of this cache serves
        rows // batch consecutive rows of the new one; max_new positions can be appended behind it.  Needs a uniform cache (lens is None).
        On a cache that already has a base (the beams of a ragged batch): the SAME base, and copies of the suffix rows, repeated like fork(rows=);
        max_new defaults to this cache's own room."""
        rows = self.batch if rows is None else rows
        assert rows % self.batch == 0
        if self.base is not None:
            base, rep = self.base, rows // self.batch
            max_new = self.max_len - self.base_len if max_new is None else max_new
            assert max_new >= self.len - self.base_len
            new = KVCache(len(self.qkv), rows, self.base_len + max_new, self.hidden, self.qkv[0].dtype, self.qkv[0].device, base=base)
            n = self.len - self.base_len
            for dst, src in zip(new.qkv, self.qkv):
                dst[:, :n] = src[:, :n].repeat_interleave(rep, dim=0) if rep > 1 else src[:, :n]
            new.len = self.len
            if self.lens is not None:
                new.lens = [l for l in self.lens for _ in range(rep)]
            return new
        if self.lens is not None:
            raise NotImplementedError("KVCache.share: the base must be uniform (rows of one length); a ragged cache can only be fork()ed")
        assert self.len > 0 and max_new is not None and max_new > 0, "KVCache.share: a non-empty base and room for new positions (max_new=)"
        return KVCache(len(self.qkv), rows, self.len + max_new, self.hidden, self.qkv[0].dtype, self.qkv[0].device, base=self)

    def row_lens(self):
        """the length of every row as a list (a uniform cache: `len`, `batch` times)"""
        return list(self.lens) if self.lens is not None else [self.len] * self.batch

    def load_row(self, slot, src, src_row=0):
        """copy the src.len positions of row `src_row` of a UNIFORM cache without a base (a prefilled video prefix) into row `slot` of this one — the
        [k | v] columns of every layer — and set that row's length; every other row keeps its length and its bytes.  `src` is only read."""
        if src.base is not None:
            raise NotImplementedError("KVCache.load_row: the source has a shared base; fork() it first")
        if self.base is not None:
            raise NotImplementedError("KVCache.load_row: a cache with a shared base holds no whole rows to load into")
        if src.lens is not None:
            raise NotImplementedError("KVCache.load_row: the source must be uniform (rows of one length)")
        n, D = src.len, self.hidden
        assert 0 <= slot < self.batch and 0 <= src_row < src.batch and n <= self.max_len and len(src.qkv) == len(self.qkv) and src.hidden == D
        assert src.qkv[0].dtype == self.qkv[0].dtype
        for dst, s in zip(self.qkv, src.qkv):
            dst[slot, :n, D:].copy_(s[src_row, :n, D:])
        lens = self.row_lens()
        lens[slot] = n
        self.set_lens(lens)

    def release(self, slot):
        """row `slot` holds nothing any more (its bytes are don't-care from here on); every other row is left alone.  On a cache with a base the row goes
        back to the base's positions: its own suffix is what it forgets."""
        assert 0 <= slot < self.batch
        lens = self.row_lens()
        lens[slot] = self.base_len
        self.truncate(lens)

    def truncate(self, n):
        """forget the positions from n on (their rows are simply overwritten by the next extend / decode_step).  n: an int for every row, or a list with
        one length per row (each at most what the row holds).  A cache with a base keeps at least the base's positions."""
        assert min(n) >= self.base_len if isinstance(n, (list, tuple)) else n >= self.base_len, "KVCache.truncate: cannot cut into the shared base"
        if isinstance(n, (list, tuple)):
            have = self.lens if self.lens is not None else [self.len] * self.batch
            assert len(n) == self.batch and all(0 <= int(a) <= h for a, h in zip(n, have))
            self.set_lens(list(n))
            return
        assert 0 <= n <= self.len
        if self.lens is not None:
            self.set_lens([min(l, n) for l in self.lens])
        else:
            self.len = n


QuantCopy = collections.namedtuple("QuantCopy", "mode dt fingerprint layers")   # LlamaModel._quant: the one quantised copy of the packed weights
# decode-weights mode -> (quantiser of a packed 16-bit weight, the hip function that multiplies by its result)
QUANT = {"int8": (pack.quant8_rows, "gemv_w8"), "int4g128": (pack.quant4_groups, "gemv_q4")}
QUANT_KEYS = ("wqkv", "wo", "wgu", "wdown")
STACK_ENTRY = os.environ.get("STLLM_STACK_ENTRY", "1") != "0"   # 0: one C-ABI call per op instead of stllm_llama_layers / stllm_vit_blocks (A/B, tests)
FUSE_NORM_ROWS = int(os.environ.get("STLLM_DECODE_FUSE_ROWS", "2"))   # decode steps with at most this many rows fuse RMSNorm into the GEMVs


class LlamaModel(nn.Module):
    def __init__(self, config, device=None):
        super().__init__()
        self.config = config
        if config.hidden_size // config.num_attention_heads != 128:
            raise NotImplementedError("RoPE epilogue / attention kernels are specialised for head_dim 128")
        self.embed_tokens = Embedding(config.vocab_size, config.hidden_size, device)
        self.layers = nn.ModuleList([LlamaDecoderLayer(config, device) for _ in range(config.num_hidden_layers)])
        self.norm = RMSNorm(config.hidden_size, config.rms_norm_eps, device)
        self._packed = {}
        self._quant = None   # QuantCopy | None: the quantised decode weights of ONE mode, per layer {wqkv, wo, wgu, wdown: (q, scale)}, built on first use
        self._rope = {}
        self._carr = {}   # C-side table of the packed layers (+ the cache it points into): rebuilt when either changes
        self._plist = ParamList(lambda: self.layers.parameters())
        self._has_lora = False   # LoraLinear modules on q_proj / v_proj (add_lora)
        self.wd_frag = True   # keep fragment-major copies of wqkv / wgu next to the packed weights (W-direct prefill GEMM); the training step switches this off:
                              # its weights change every step and its taped forward does not use the copies

    def pack(self, dtype=None):
        dt = hip.torch_dtype(dtype) if dtype is not None else runtime.compute_dtype()
        fp = params_fingerprint(self._plist.get())   # a stale packed copy after p.data.copy_ / .to(device) would run silently
        fp = fp + (tuple(lora_mod.adapters_of(l) is not None for l in self.layers),) if self._has_lora else fp   # merged / unmerged adapters pack differently
        hit = self._packed.get(dt)
        if hit is None or hit[0] != fp:
            self._packed = {}  # one packed copy at a time (13.5 GB at 7B) ...
            self._carr = {}    # ... including the C-side table, which holds a reference to the list it was built from
            # adapters whose B is all zero (peft's init: a fresh model) add exact zeros: pack — and run — the base path, bit for bit the model without adapters
            lora = self.lora_active() and lora_mod.any_nonzero_b(self)   # (one device read per pack miss)
            hit = (fp, [l.pack(dt, self.config.num_attention_heads, frag=self.wd_frag, lora=lora) for l in self.layers])
            self._packed[dt] = hit
        return hit[1]

    def pack_quant(self, mode, dtype=None):
        """the quantised decode weights of `mode` (a key of QUANT): per layer {wqkv, wo, wgu, wdown} -> (q, scale), quantised from the packed 16-bit
        weights of pack(dt) (so the RoPE / gate-up row orders are inherited) and cached under the same parameter fingerprint (layers.params_fingerprint:
        `_version` + `data_ptr()`): rebuilt, like the 16-bit pack, after an in-place edit of a master (p.copy_, p.mul_, an optimizer step through
        torch), load_state_dict or .to(device); a write through `p.data` or through a raw pointer bumps no version counter — such writers call
        repack(), which drops both.  ONE slot: building a copy drops the one of another mode or dtype; the first decode_step that sees another mode
        (None included) drops it too."""
        dt = hip.torch_dtype(dtype) if dtype is not None else runtime.compute_dtype()
        layers = self.pack(dt)
        fp = self._packed[dt][0]
        if self._quant is None or self._quant[:3] != (mode, dt, fp):
            self._quant = None   # free the old copy before the new one is built
            quant = QUANT[mode][0]
            self._quant = QuantCopy(mode, dt, fp, [{k: quant(pk[k]) for k in QUANT_KEYS} for pk in layers])
        return self._quant.layers

    def pack_w8(self, dtype=None):
        """the int8 decode weights (pack_quant): (q int8 [N, K], scale f32 [N]) = pack.quant8_rows of every packed projection weight.  + 6.6 GB at 7B."""
        return self.pack_quant("int8", dtype)

    def pack_q4(self, dtype=None):
        """the 4-bit decode weights (pack_quant): (qp uint8 [N, K / 2], scale f32 [N, K / 128]) = pack.quant4_groups.  + 3.5 GB at 7B."""
        return self.pack_quant("int4g128", dtype)

    def add_lora(self, r, lora_alpha=32):
        """peft's get_peft_model for target_modules = [q_proj, v_proj] (st_llm.py:165-177): fresh adapters (B = 0) on every decoder layer"""
        lora_mod.add_adapters(self, r, lora_alpha)
        self._has_lora = True

    def lora_active(self):
        return self._has_lora and any(lora_mod.adapters_of(l) is not None for l in self.layers)

    def repack_adapters(self):
        """after an optimizer step on the adapters alone (the kernels write the masters behind torch's version counters): refresh A and the P extra
        columns of the packed QKV weights IN PLACE — the frozen base weights (13 GB at 7B) are not cast again, the C-side tables stay valid.
        A pack made while B was still all zero has no extra columns: that one is dropped and rebuilt once."""
        for dt, (fp, layers) in list(self._packed.items()):
            if "lora_A" not in layers[0]:
                self.repack()
                return
            for l, pk in zip(self.layers, layers):
                lora_mod.refresh_qkv(pk, *lora_mod.adapters_of(l), dt, self.config.num_attention_heads)

    def repack(self):
        """drop every copy made from the parameters: the 16-bit pack, the quantised copy, the C-side table, the parameter list"""
        self._packed = {}
        self._quant = None
        self._carr = {}
        self._plist.reset()

    def _load_from_state_dict(self, *a, **k):
        self.repack()
        return super()._load_from_state_dict(*a, **k)

    def rope(self, S, device):
        """cos / sin tables [S, 64] on the device, cached per (S, device) — a handful of entries, oldest dropped.  The MVM forward alternates
        two sequence lengths inside ONE step (masked and un-masked prefill, st_llm.py:56-92): with a single-entry cache (rounds 1-3) every
        prefill rebuilt the tables on the host and copied them from pageable memory — a device synchronisation that cost configs c4 / c5
        40-50 ms of idle GPU per step (profiles/r04_mvm_host_stall.md)."""
        key = (S, str(device))
        hit = self._rope.get(key)
        if hit is None:
            d = self.config.hidden_size // self.config.num_attention_heads
            hit = pack.rope_tables(S, d, self.config.rope_theta, device)
            if len(self._rope) >= 8:
                self._rope.pop(next(iter(self._rope)))
            self._rope[key] = hit
        return hit

    def prefill(self, inputs_embeds, attention_mask=None, cache=None):
        """inputs_embeds f32 [B,S,D]; attention_mask [B,S] (1 = token, right-padded) or None; cache: KVCache to fill.
        Returns (hidden f32 [B,S,D] after model.norm == hidden_states[-1], hidden in compute dtype [B*S,D])."""
        cfg = self.config
        dt = runtime.compute_dtype()
        layers = self.pack(dt)
        B, S, D = inputs_embeds.shape
        H = cfg.num_attention_heads
        hd = D // H
        dev = inputs_embeds.device
        x = inputs_embeds.reshape(B * S, D).float().clone()
        kv_len = None
        row_lens = None
        if attention_mask is not None:
            m = hip.host_mask(attention_mask).long()   # the assembler built it on the host: no D2H read, no stall
            if not bool((m[:, 1:] <= m[:, :-1]).all()):
                raise NotImplementedError("only right-padded attention masks occur on this path (st_llm.py:400-404)")
            if int(m.sum()) != m.numel():
                row_lens = m.sum(dim=1).to(torch.int32)
                kv_len = hip.h2d(row_lens, dev)
        cos, sin = self.rope(S, dev)
        if cache is not None:
            if cache.base is not None:
                raise NotImplementedError("prefill into a KV cache with a shared base: its first positions are the base's (extend / decode_step append behind them)")
            assert cache.batch == B and cache.max_len >= S and cache.qkv[0].dtype == dt
            cache.len = S
            # a right-padded batch fills a RAGGED cache: the fused rows land where they always do, kv_len masks the pad keys as on the no-cache path, the pad
            # positions hold don't-care rows that later steps overwrite
            cache.set_lens(row_lens.tolist() if row_lens is not None else None)
        # the 32-layer loop is ONE call into the C ABI (stllm_llama_layers; == prefill_layer_by_layer, bit for bit); with a cache the
        # fused QKV rows of every layer are written straight into its cache buffer (rows (b, s) at b * max_len + s)
        if cache is not None:
            carr = hip.llama_layer_array(layers, cache)       # once per generate(): not worth caching (and it would pin the cache)
        else:
            if self._carr.get("layers") is not layers:
                self._carr = {"layers": layers, "carr": hip.llama_layer_array(layers)}
            carr = self._carr["carr"]
        if STACK_ENTRY:
            kw = {}
            if "lora_A" in layers[0]:   # active adapters: stllm_llama_layers_lora, still one C call
                if self._carr.get("lora_of") is not layers:
                    self._carr.update(lora_of=layers, lora=hip.llama_lora_array(layers))
                kw["lora"] = self._carr["lora"]
            hip.llama_layers(x, layers, carr, B=B, S=S, n_heads=H, eps=cfg.rms_norm_eps, rope=(cos, sin), dtype=dt, kv_len=kv_len, cache=cache, **kw)
        else:
            self.prefill_layers_per_op(x, layers, B, S, cos, sin, kv_len, cache, dt)
        h16, h32 = hip.rmsnorm(x, self.norm.weight, cfg.rms_norm_eps, dtype=dt, want_f32=True)
        return h32.view(B, S, D), h16

    def prefill_layers_per_op(self, x, layers, B, S, cos, sin, kv_len, cache, dt):
        """The decoder-layer loop as one C-ABI call per op — what stllm_llama_layers issues from C.  Kept as the reference the stack
        entry point is tested against (-m gpu: bit-identical) and as the body the test-only CPU contract backend runs."""
        D, H = self.config.hidden_size, self.config.num_attention_heads
        hd = D // H
        strides = None if cache is None else cache.kv(0)[2]

        def qkv_to(li):   # the cache buffer is the GEMM's output: rows (b, s) at b*max_len + s
            return {} if cache is None else dict(out=cache.flat(li), M=B * S, o_rows=(S, strides[0]))

        def attn(li, qkv):
            return hip.attention(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], B=B, H=H, Sq=S, Skv=S, D=hd,
                                 scale=hd ** -0.5, causal=True, kv_len=kv_len, q_strides=strides, k_strides=strides,
                                 v_strides=strides)
        proj = gemm_proj(layers, dt, True)
        for li, pk in enumerate(layers):
            decoder_layer(self, dt, x, pk, li, proj=proj, qkv_to=qkv_to, attn=attn, rope=(cos, sin), rope_seq=S)
        return x

    def extend(self, inputs_embeds, cache, lengths=None):
        """S new positions behind the P = cache.len positions the cache already holds, in ONE pass through the decoder layers (a question behind a
        prefilled video; forward(past_key_values=...) runs decode_step once per token instead).  inputs_embeds f32 [B,S,D].  Per layer: RMSNorm ->
        QKV GEMM + RoPE at the positions P .. P+S-1, written into rows [P, P+S) of the layer's cache buffer -> causal attention of the S query rows over
        the P+S cached keys with the query offset P (hip.attention(q_off=P)) -> o_proj -> MLP.  Sets cache.len = P + S; returns what prefill returns.
        P = 0 is prefill(cache=cache).  bf16 / fp16 / fp32; the split modes (bf16x3 / mixed) are not wired.
        lengths: suffixes of different lengths S_b <= S, right-padded to S, behind a uniform prefix — the cache becomes ragged (lens = P + S_b), the pad query
        rows are don't-care.  Runs the per-op body on hip.attention(q_off=P, kv_len=P + S_b).
        A RAGGED cache (cache.lens set), or a row with lengths[b] == 0, takes extend_ragged: row b appends its 0 <= S_b <= S tokens behind its own P_b
        positions, a row with S_b == 0 is left exactly as it is."""
        cfg = self.config
        dt = runtime.compute_dtype()
        if runtime.gemm_split():
            raise NotImplementedError("LlamaModel.extend runs in the bf16 / fp16 / fp32 modes; the bf16x3 / mixed modes have no extend path")
        B, S, D = inputs_embeds.shape
        P = cache.len
        assert cache.batch == B and cache.qkv[0].dtype == dt
        if lengths is not None:
            lengths = [int(n) for n in lengths]
            assert len(lengths) == B and all(0 <= n <= S for n in lengths)
        if cache.lens is not None or (lengths is not None and min(lengths) == 0):
            return self.extend_ragged(inputs_embeds, cache, lengths)
        assert P + S <= cache.max_len, "KV cache full"
        if lengths is not None and len(set(lengths)) == 1 and lengths[0] == S:
            lengths = None
        if P == 0:   # (a cache with a base holds P > 0 positions)
            mask = None if lengths is None else (torch.arange(S)[None, :] < torch.tensor(lengths)[:, None]).long()
            return self.prefill(inputs_embeds, mask, cache=cache)
        layers = self.pack(dt)
        x = inputs_embeds.reshape(B * S, D).float().clone()
        cos, sin = self.rope(cache.max_len, inputs_embeds.device)
        cos, sin = cos[P:P + S], sin[P:P + S]
        if cache.base is not None:   # a shared base: the per-op body on hip.attention_shared (the one-call C stack entry does not know about bases)
            self.extend_layers_shared(x, layers, B, S, P, cos, sin, cache, dt, lengths)
        elif lengths is not None:
            kv_len = hip.h2d(torch.tensor([P + n for n in lengths], dtype=torch.int32), inputs_embeds.device)
            self.extend_layers_per_op(x, layers, B, S, P, cos, sin, cache, dt, kv_len=kv_len)
        elif STACK_ENTRY and "lora_A" not in layers[0]:
            hip.llama_layers_extend(x, layers, hip.llama_layer_array(layers, cache), B=B, S=S, pos0=P, n_heads=cfg.num_attention_heads, eps=cfg.rms_norm_eps,
                                    rope=(cos, sin), dtype=dt, cache=cache)
        else:
            self.extend_layers_per_op(x, layers, B, S, P, cos, sin, cache, dt)
        cache.len = P + S
        if lengths is not None:
            cache.set_lens([P + n for n in lengths])
        h16, h32 = hip.rmsnorm(x, self.norm.weight, cfg.rms_norm_eps, dtype=dt, want_f32=True)
        return h32.view(B, S, D), h16

    def extend_layers_per_op(self, x, layers, B, S, P, cos, sin, cache, dt, kv_len=None):
        """extend's layer loop as one C-ABI call per op — what stllm_llama_layers_extend issues from C (bit-identical), the body active LoRA adapters
        run, and the one the test-only CPU contract backend runs"""
        D, H = self.config.hidden_size, self.config.num_attention_heads
        hd = D // H
        kv = {"kv_len": kv_len} if kv_len is not None else {}
        strides = cache.kv(0)[2]

        def qkv_to(li):   # row (b, s) of the suffix at b * max_len + P + s
            return dict(out=cache.flat(li)[P:], M=B * S, o_rows=(S, strides[0]))

        def attn(li, new):
            k, v, _ = cache.kv(li)
            return hip.attention(new[:, :D], k, v, B=B, H=H, Sq=S, Skv=P + S, D=hd, scale=hd ** -0.5, causal=True,
                                 q_strides=strides, k_strides=strides, v_strides=strides, q_off=P, **kv)
        proj = gemm_proj(layers, dt, True)
        for li, pk in enumerate(layers):
            decoder_layer(self, dt, x, pk, li, proj=proj, qkv_to=qkv_to, attn=attn, rope=(cos, sin), rope_seq=S)
        return x

    def extend_ragged(self, inputs_embeds, cache, lengths=None):
        """extend on a ragged cache: row b appends lengths[b] = S_b tokens (0 <= S_b <= S, right-padded to S; None: S for every row) behind the P_b positions it
        holds (cache.lens[b], or cache.len).  The per-op decoder_layer body: the QKV GEMM + RoPE writes a dense [B * S, 3D] scratch — RoPE rows cos / sin[P_b + i],
        gathered once per call, rope_seq = B * S —, hip.kv_append_spans copies the [k | v] columns of the live rows to positions P_b .. P_b + S_b - 1 of the cache,
        hip.attention_offset_ragged reads q from the scratch and K / V from the cache (never behind P_b + S_b).  A row with S_b == 0 is untouched: nothing of
        it is written, its K / V are not read.  The pad rows of the returned hidden states are don't-care but finite.  Sets cache.lens = P_b + S_b."""
        cfg = self.config
        dt = runtime.compute_dtype()
        B, S, D = inputs_embeds.shape
        H = cfg.num_attention_heads
        hd = D // H
        dev = inputs_embeds.device
        if cache.base is not None:
            raise NotImplementedError("LlamaModel.extend behind a ragged prefix on a shared base (rows of different lengths, or a row that appends nothing): "
                                      "fork() the cache first")
        if not hip.ragged_extend_available(dev):
            raise NotImplementedError("LlamaModel.extend behind a ragged prefix (rows of different lengths, or a row that appends nothing) needs "
                                      "hip.attention_offset_ragged / hip.kv_append_spans, which this backend does not provide for " + str(dev) +
                                      ": append one token at a time with decode_step")
        have = list(cache.lens) if cache.lens is not None else [cache.len] * B
        new = [S] * B if lengths is None else lengths
        assert all(p + n <= cache.max_len for p, n in zip(have, new)), "KV cache full"
        layers = self.pack(dt)
        x = inputs_embeds.reshape(B * S, D).float().clone()
        cos, sin = self.rope(cache.max_len, dev)
        # the pad rows take any valid position: the row's own next ones, clamped below max_len
        pos = hip.h2d(torch.tensor([min(p + i, cache.max_len - 1) for p in have for i in range(S)], dtype=torch.int32), dev)
        cos, sin = hip.gather_rows(cos, pos), hip.gather_rows(sin, pos)
        q_off = hip.h2d(torch.tensor(have, dtype=torch.int32), dev)
        n_new = hip.h2d(torch.tensor(new, dtype=torch.int32), dev)
        kv_len = hip.h2d(torch.tensor([p + n for p, n in zip(have, new)], dtype=torch.int32), dev)
        max_kv = max(1, max(p + n for p, n in zip(have, new)))
        dense = torch.empty((B * S, 3 * D), device=dev, dtype=dt)
        strides = cache.kv(0)[2]

        def attn(li, dense):
            hip.kv_append_spans(dense, cache.qkv[li], q_off, n_new, S=S)
            k, v, _ = cache.kv(li)
            return hip.attention_offset_ragged(dense[:, :D], k, v, q_off, kv_len, B=B, H=H, Sq=S, max_kv=max_kv, D=hd, scale=hd ** -0.5,
                                               q_strides=(S * 3 * D, 3 * D), k_strides=strides, v_strides=strides)
        proj = gemm_proj(layers, dt, True)
        for li, pk in enumerate(layers):
            decoder_layer(self, dt, x, pk, li, proj=proj, qkv_to=lambda li: {"out": dense}, attn=attn, rope=(cos, sin), rope_seq=B * S)
        cache.set_lens([p + n for p, n in zip(have, new)])
        h16, h32 = hip.rmsnorm(x, self.norm.weight, cfg.rms_norm_eps, dtype=dt, want_f32=True)
        return h32.view(B, S, D), h16

    def step_segments(self, embeds, cache, segments):
        """One pass through the decoder layers over a PACKED step: embeds f32 [T, D] is the concatenation of the segments' tokens,
        segments a list of (slot, n) in packed order — n >= 1 tokens appended behind the cache.lens[slot] positions that row `slot` of `cache` holds (one
        token for a running request, a whole prompt for a newly admitted one; slots distinct).  Per layer: RMSNorm -> QKV GEMM + RoPE into a dense [T, 3D]
        scratch (RoPE rows gathered at lens[slot] + i, rope_seq = T) -> hip.kv_append_segments -> hip.attention_segments -> o_proj -> MLP.  No pad rows
        anywhere: T GEMM rows, T query rows.  Sets the length of every named slot to lens + n; a slot that is not named keeps its length and its bytes.
        Returns the final-norm hidden rows of every segment's LAST token only: (f32 [R, D], compute dtype [R, D]).  bf16 / fp16 / fp32; the split
        modes and quantised decode weights raise (the quantised modes serve pure-decode steps through decode_step).  A cache with a base (one base row)
        takes step_segments_shared: the same contract, the base's K / V read once for all packed rows."""
        cfg = self.config
        dt = runtime.compute_dtype()
        if runtime.gemm_split():
            raise NotImplementedError("LlamaModel.step_segments runs in the bf16 / fp16 / fp32 modes; the bf16x3 / mixed modes have no segment path")
        if runtime.decode_weights() is not None:
            raise NotImplementedError(f"LlamaModel.step_segments streams the 16-bit weights: {runtime.decode_weights()} decode weights serve decode_step only")
        T, D = embeds.shape
        H = cfg.num_attention_heads
        hd = D // H
        dev = embeds.device
        if cache.base is not None:
            return self.step_segments_shared(embeds, cache, segments)
        if not hip.segments_available(dev):
            raise NotImplementedError("LlamaModel.step_segments needs hip.attention_segments / hip.kv_append_segments, which this backend does not provide for " +
                                      str(dev))
        segments = [(int(s), int(n)) for s, n in segments]
        slots, new = [s for s, _ in segments], [n for _, n in segments]
        assert segments and len(set(slots)) == len(slots) and all(0 <= s < cache.batch for s in slots), "step_segments: slots must be distinct and in range"
        assert min(new) >= 1 and sum(new) == T, "step_segments: every segment carries at least one token and the segments cover the packed rows"
        assert cache.qkv[0].dtype == dt
        lens = cache.row_lens()
        have = [lens[s] for s in slots]
        assert all(p + n <= cache.max_len for p, n in zip(have, new)), "KV cache full"
        row0 = [sum(new[:r]) for r in range(len(new))]
        layers = self.pack(dt)
        x = embeds.float().clone()
        cos, sin = self.rope(cache.max_len, dev)

        def tab(v):
            return hip.h2d(torch.tensor(v, dtype=torch.int32), dev)
        pos = tab([p + i for p, n in zip(have, new) for i in range(n)])
        cos, sin = hip.gather_rows(cos, pos), hip.gather_rows(sin, pos)
        slot_t, row0_t, q_off, n_new, kv_len = tab(slots), tab(row0), tab(have), tab(new), tab([p + n for p, n in zip(have, new)])
        max_n, max_kv = max(new), max(p + n for p, n in zip(have, new))
        dense = torch.empty((T, 3 * D), device=dev, dtype=dt)
        strides = cache.kv(0)[2]

        def attn(li, dense):
            hip.kv_append_segments(dense, cache.qkv[li], slot_t, row0_t, q_off, n_new, T=T, max_n=max_n)
            k, v, _ = cache.kv(li)
            return hip.attention_segments(dense[:, :D], k, v, slot_t, row0_t, q_off, kv_len, H=H, D=hd, T=T, n_slots=cache.batch, max_n=max_n, max_kv=max_kv,
                                          scale=hd ** -0.5, k_strides=strides, v_strides=strides)
        proj = gemm_proj(layers, dt, True)
        for li, pk in enumerate(layers):
            decoder_layer(self, dt, x, pk, li, proj=proj, qkv_to=lambda li: {"out": dense}, attn=attn, rope=(cos, sin), rope_seq=T)
        for s, p, n in zip(slots, have, new):
            lens[s] = p + n
        cache.set_lens(lens)
        last = hip.gather_rows(x, tab([r0 + n - 1 for r0, n in zip(row0, new)]))
        h16, h32 = hip.rmsnorm(last, self.norm.weight, cfg.rms_norm_eps, dtype=dt, want_f32=True)
        return h32, h16

    def step_segments_shared(self, embeds, cache, segments):
        """step_segments on a cache with a shared base (KVCache.share of ONE base row; reached through step_segments, which has checked the
        modes): the same contract.  RoPE rows are gathered at the TOTAL positions lens[slot] + i; the append and the attention work on the cache's own
        [slots, max_len - P, 3D] buffers at the LOCAL positions lens[slot] - P — hip.kv_append_segments, then hip.attention_segments_shared, which reads the
        base's P keys once for all T packed rows and every segment's own suffix.  The base's buffers are only read."""
        cfg = self.config
        dt = runtime.compute_dtype()
        T, D = embeds.shape
        H = cfg.num_attention_heads
        hd = D // H
        dev = embeds.device
        P = cache.base_len
        if cache.base.batch != 1:
            raise NotImplementedError(f"LlamaModel.step_segments on a KV cache with a shared base of {cache.base.batch} rows: one base row (one video) only; "
                                      "fork() it first")
        if not hip.segments_shared_available(dev):
            raise NotImplementedError("LlamaModel.step_segments on a KV cache with a shared base needs hip.attention_segments_shared / hip.kv_append_segments, "
                                      "which this backend does not provide for " + str(dev))
        segments = [(int(s), int(n)) for s, n in segments]
        slots, new = [s for s, _ in segments], [n for _, n in segments]
        assert segments and len(set(slots)) == len(slots) and all(0 <= s < cache.batch for s in slots), "step_segments: slots must be distinct and in range"
        assert min(new) >= 1 and sum(new) == T, "step_segments: every segment carries at least one token and the segments cover the packed rows"
        assert cache.qkv[0].dtype == dt and cache.base.qkv[0].dtype == dt
        lens = cache.row_lens()
        have = [lens[s] for s in slots]
        assert all(p + n <= cache.max_len for p, n in zip(have, new)), "KV cache full"
        row0 = [sum(new[:r]) for r in range(len(new))]
        layers = self.pack(dt)
        x = embeds.float().clone()
        cos, sin = self.rope(cache.max_len, dev)

        def tab(v):
            return hip.h2d(torch.tensor(v, dtype=torch.int32), dev)
        pos = tab([p + i for p, n in zip(have, new) for i in range(n)])
        cos, sin = hip.gather_rows(cos, pos), hip.gather_rows(sin, pos)
        off = [p - P for p in have]                                   # suffix-local from here on
        slot_t, row0_t, sfx_off, n_new, sfx_len = tab(slots), tab(row0), tab(off), tab(new), tab([p + n for p, n in zip(off, new)])
        max_n, max_sfx = max(new), max(p + n for p, n in zip(off, new))
        dense = torch.empty((T, 3 * D), device=dev, dtype=dt)

        def attn(li, dense):
            hip.kv_append_segments(dense, cache.qkv[li], slot_t, row0_t, sfx_off, n_new, T=T, max_n=max_n)
            (kp, vp, kp_strides), (ks, vs, ks_strides) = cache.base.kv(li), cache.kv(li)
            return hip.attention_segments_shared(dense[:, :D], kp, vp, ks, vs, slot_t, row0_t, sfx_off, sfx_len, H=H, D=hd, T=T, P=P, n_slots=cache.batch,
                                                 max_n=max_n, max_sfx=max_sfx, scale=hd ** -0.5, kp_strides=kp_strides, ks_strides=ks_strides)
        proj = gemm_proj(layers, dt, True)
        for li, pk in enumerate(layers):
            decoder_layer(self, dt, x, pk, li, proj=proj, qkv_to=lambda li: {"out": dense}, attn=attn, rope=(cos, sin), rope_seq=T)
        for s, p, n in zip(slots, have, new):
            lens[s] = p + n
        cache.set_lens(lens)
        last = hip.gather_rows(x, tab([r0 + n - 1 for r0, n in zip(row0, new)]))
        h16, h32 = hip.rmsnorm(last, self.norm.weight, cfg.rms_norm_eps, dtype=dt, want_f32=True)
        return h32, h16

    def extend_layers_shared(self, x, layers, B, S, pos, cos, sin, cache, dt, lengths=None):
        """extend's layer loop for a cache with a shared base (KVCache.share): the S new rows sit at the local positions [off, off + S), off = pos - base_len,
        of the cache's own buffers.  The QKV GEMM writes a dense [B * S, 3D] buffer — the 16-bit kernels behind hip.attention_shared walk the R * S query
        rows of a group at ONE row stride — whose rows are then copied into the cache; the attention reads the base's P keys once per group and row b's own
        off + S_b suffix keys (causal with the query offset `off`)."""
        D, H = self.config.hidden_size, self.config.num_attention_heads
        hd = D // H
        P = cache.base_len
        off = pos - P
        dev = x.device
        sfx_len = None if lengths is None else hip.h2d(torch.tensor([off + n for n in lengths], dtype=torch.int32), dev)
        dense = torch.empty((B * S, 3 * D), device=dev, dtype=dt)

        def attn(li, dense):
            cache.qkv[li][:, off:off + S].copy_(dense.view(B, S, 3 * D))
            (kp, vp, kp_strides), (ks, vs, ks_strides) = cache.base.kv(li), cache.kv(li)
            return hip.attention_shared(dense[:, :D], kp, vp, ks, vs, B=B, G=cache.base.batch, H=H, Sq=S, P=P, D=hd,
                                        scale=hd ** -0.5, max_sfx=off + S, sfx_len=sfx_len, sfx_q_off=off, causal=True, q_strides=(S * 3 * D, 3 * D),
                                        kp_strides=kp_strides, ks_strides=ks_strides)
        proj = gemm_proj(layers, dt, True)
        for li, pk in enumerate(layers):
            decoder_layer(self, dt, x, pk, li, proj=proj, qkv_to=lambda li: {"out": dense}, attn=attn, rope=(cos, sin), rope_seq=S)
        return x

    def qkv_operand(self, x, pk, dt):
        """the A operand of a layer's QKV GEMM: RMSNorm(x) in the compute dtype; with active adapters the rows carry P more columns,
        t = h [A_q ; A_v]^T and a zero pad (stllm_lora_down), matching the K-extended weight"""
        cfg = self.config
        M, D = x.shape
        buf = torch.empty((M, D + pk["lora_P"]), device=x.device, dtype=dt)
        hip.rmsnorm(x, pk["ln1"], cfg.rms_norm_eps, dtype=dt, out_t=buf[:, :D])
        hip.lora_down(buf[:, :D], pk["lora_A"], dtype=dt, out=buf[:, D:])
        return buf

    def sp_layer_part(self, part, x, layers, li, qkv, s0, s1, cos_l, sin_l, dt, carr):
        """one half of a decoder layer on this rank's rows [s0, s1) (prefill_sp): part 0 = RMSNorm + QKV GEMM + RoPE into qkv[s0:s1], part 1 = attention over
        the s1 rows + o_proj + RMSNorm + gate/up + down.  carr: the C-side layer table (one stllm_llama_layer_sp call) or None (the per-op body)."""
        cfg = self.config
        D, H = cfg.hidden_size, cfg.num_attention_heads
        hd = D // H
        pk = layers[li]
        if carr is not None:
            return hip.llama_layer_sp(x, carr, li, qkv, s0=s0, s1=s1, part=part, n_heads=H, eps=cfg.rms_norm_eps, rope=(cos_l, sin_l), dtype=dt,
                                      inter=pk["wgu"].shape[0] // 2)

        def attn(li, qkv):   # over all s1 rows; o_proj takes this rank's
            return hip.attention(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], B=1, H=H, Sq=s1, Skv=s1, D=hd, scale=hd ** -0.5, causal=True)[s0:s1]
        decoder_layer(self, dt, x, pk, li, proj=gemm_proj(layers, dt, True), qkv_to=lambda li: {"out": qkv[s0:s1]}, attn=attn, rope=(cos_l, sin_l),
                      rope_seq=s1 - s0, part=part, qkv=qkv)
        return x

    def prefill_sp(self, inputs_embeds, sp):
        """Sequence-parallel prefill of ONE sequence inside a clip team (stllm_amd.parallel, round 5): this rank runs the decoder layers on the
        positions [s0, s1) = parallel.sp_row_ranges(S, k)[j] only.  Causal attention makes the team's dependency one-directional: per layer the
        K | V rows of the members before this one arrive point-to-point (posted before this rank's own QKV GEMM, awaited in front of its
        attention), its own K | V rows leave for the members behind it right after the QKV GEMM — the transfers ride under the o_proj / MLP
        GEMMs of the sender and the RMSNorm / QKV GEMM of the receiver.  No kernel knows about any of this: the fused QKV buffer simply has rows
        [0, s1) — foreign K | V, own q | k | v — and the attention runs causal over s1 x s1 (the s0 foreign query rows are zero, their outputs unused:
        +7 us per layer at S = 580, k = 2, against a second set of attention kernels with a query offset).
        sp: dict(index=j, size=k, ranks=[global ranks of the team], rank=this rank, group=None, mailbox=None | parallel.Mailbox).
        inputs_embeds f32 [1, S, D] (every member assembles the whole sequence: one 9.5 MB gather).  Returns (hidden f32 [1, s1 - s0, D] after
        model.norm, the same rows in the compute dtype, (s0, s1))."""
        from .. import parallel
        cfg = self.config
        dt = runtime.compute_dtype()
        if self.lora_active():
            raise NotImplementedError("sequence-parallel prefill with active LoRA adapters: merge_adapter() first")
        layers = self.pack(dt)
        B, S, D = inputs_embeds.shape
        if B != 1:
            raise NotImplementedError("sequence-parallel prefill: one sequence per team (stllm_amd.parallel.TeamPlan)")
        H = cfg.num_attention_heads
        hd = D // H
        dev = inputs_embeds.device
        j, k, ranks, me, group, box = sp["index"], sp["size"], sp["ranks"], sp["rank"], sp.get("group"), sp.get("mailbox")
        rr = parallel.sp_row_ranges(S, k)
        s0, s1 = rr[j]
        x = inputs_embeds.reshape(S, D)[s0:s1].float().clone()
        cos, sin = self.rope(S, dev)
        cos_l, sin_l = cos[s0:s1], sin[s0:s1]
        qkv = torch.empty((s1, 3 * D), device=dev, dtype=dt)
        if s0 > 0:
            qkv[:s0, :D].zero_()          # query columns of the foreign rows: never written again, their attention outputs are never read
        n_loc = s1 - s0
        if n_loc == 0:                     # more members than 32-row groups: this member has no rows (and nobody waits for any from it)
            return x.view(1, 0, D), x.to(dt), (s0, s1)
        pending = []                       # send handles + the packed buffers they read: kept until the end of the prefill
        # round 6 (VERDICT r05 missing #4): the two halves of a layer — up to the QKV rows, and from the attention on — are ONE C call each
        # (stllm_llama_layer_sp) instead of 2 + 5 per-op calls; the split verify mode and STACK_ENTRY = 0 keep the per-op body (bit-identical)
        carr = None
        if STACK_ENTRY and not runtime.gemm_split():
            if self._carr.get("layers") is not layers:
                self._carr = {"layers": layers, "carr": hip.llama_layer_array(layers)}
            carr = self._carr["carr"]
        for li_, pk in enumerate(layers):
            recvs = [(torch.empty((rr[i][1] - rr[i][0], 2 * D), device=dev, dtype=dt), ranks[i], ("kv", li_)) for i in range(j) if rr[i][1] > rr[i][0]]
            works = parallel.p2p_exchange([], recvs, me, group, box) if recvs else []
            self.sp_layer_part(0, x, layers, li_, qkv, s0, s1, cos_l, sin_l, dt, carr)
            later = [i for i in range(j + 1, k) if rr[i][1] > rr[i][0]]
            if later:
                kv = qkv[s0:s1, D:].contiguous()
                pending.append((kv, parallel.p2p_exchange([(kv, ranks[i], ("kv", li_)) for i in later], [], me, group, box)))
            for w in works:
                w.wait()
            for (buf, _, _), i in zip(recvs, [i for i in range(j) if rr[i][1] > rr[i][0]]):
                qkv[rr[i][0]:rr[i][1], D:].copy_(buf)
            self.sp_layer_part(1, x, layers, li_, qkv, s0, s1, cos_l, sin_l, dt, carr)
        for _, ws in pending:
            for w in ws:
                w.wait()
        h16, h32 = hip.rmsnorm(x, self.norm.weight, cfg.rms_norm_eps, dtype=dt, want_f32=True)
        return h32.view(1, n_loc, D), h16, (s0, s1)

    def decode_step(self, x_new, cache):
        """One token per sequence: x_new f32 [B,1,D] (embedding of the token at position cache.len).  Appends its K/V to the
        cache and returns (hidden f32 [B,1,D] after model.norm, hidden compute-dtype [B,D])."""
        cfg = self.config
        dt = runtime.compute_dtype()
        wmode = runtime.decode_weights()
        if wmode is not None and dt == torch.float32:
            raise NotImplementedError(f"{wmode} decode weights need a 16-bit compute mode (bf16 / fp16), not {runtime.mode_name()!r}")
        if cache.base is not None and runtime.gemm_split():
            raise NotImplementedError("decode_step on a KV cache with a shared base runs in the bf16 / fp16 / fp32 modes; fork() it for bf16x3 / mixed")
        layers = self.pack(dt)
        B, _, D = x_new.shape
        qw = None
        if wmode is not None:
            if "lora_A" in layers[0]:
                raise NotImplementedError(f"{wmode} decode weights with active LoRA adapters: merge_adapter() first")
            if B <= 16:   # the decode regime of hip.gemv_w8 / hip.gemv_q4; larger batches stream the 16-bit weights on the tile kernels
                qw = self.pack_quant(wmode, dt)
        if self._quant is not None and self._quant.mode != wmode:
            self._quant = None   # the mode was switched away: free the quantised copy
        pos = cache.len
        assert pos < cache.max_len, "KV cache full"
        cos, sin = self.rope(cache.max_len, x_new.device)
        cpos, spos = cos[pos:pos + 1], sin[pos:pos + 1]
        rs, rg = 1, None
        if cache.base is not None or cache.lens is not None:
            # ragged step: token b sits at position lens[b].  The RoPE epilogues take pos = row % rope_seq, so B table rows cos[lens[b]] with rope_seq = B
            # need no GEMV change; the positions / lengths travel through the pinned ring (the host knows them: no device synchronisation).  The QKV
            # GEMV writes rows at ONE stride only -> a dense [B, 3D] scratch row, scattered into the cache by kv_append_rows (decode_attn).
            # A shared base ALWAYS takes this route (one path for uniform and ragged suffixes): RoPE at the total positions, the [k | v] columns appended
            # at the LOCAL position lens[b] - P of the cache's own buffers, attention through hip.attention_shared (decode_attn)
            dev = x_new.device
            assert cache.batch == B
            lens_, P_ = cache.lens or [pos] * B, cache.base_len
            pos_d = hip.h2d(torch.tensor(lens_, dtype=torch.int32), dev)
            cpos, spos = hip.gather_rows(cos, pos_d), hip.gather_rows(sin, pos_d)
            rs = B
            # without a base the local positions ARE the total ones: the table just uploaded serves as both
            rg = dict(pos=pos_d if cache.base is None else hip.h2d(torch.tensor([n - P_ for n in lens_], dtype=torch.int32), dev),
                      kv_len=hip.h2d(torch.tensor([n - P_ + 1 for n in lens_], dtype=torch.int32), dev), max_kv=pos - P_ + 1,
                      scratch=torch.empty((B, 3 * D), device=dev, dtype=dt))
        x = x_new.reshape(B, D).float().clone()
        # 16-bit modes, <= 8 rows: both RMSNorms ride inside the GEMV that consumes them (2 launches per layer fewer)
        # (every workgroup of the GEMV recomputes the norm of all its rows: worth it for 1-2 rows — 3.70 -> 3.29 ms/token —, a loss for
        #  the 5 rows of beam search, where 2752 workgroups x 6 staged rows re-read 0.5 GB through L2)
        fuse = dt != torch.float32 and B <= FUSE_NORM_ROWS
        if qw is None:
            proj = gemm_proj(layers, dt, False)
        else:   # the same step over the quantised weights (W8A16 / W4A16 kernels): same epilogues, same fused norms
            fuse = fuse and B <= 2   # (stllm_gemv_w8 / stllm_gemv_q4 fuse the norm for <= 2 rows)
            fn = QUANT[wmode][1]

            def proj(li, key, a, **kw):
                return getattr(hip, fn)(a, *qw[li][key], dtype=dt, **kw)

        def qkv_to(li):   # [B, 3D]: row `pos` of the layer's cache buffer, a view with the row stride max_len*3D | the dense scratch
            return {"out": cache.qkv[li][:, pos] if rg is None else rg["scratch"]}

        def attn(li, row):
            return self.decode_attn(row, cache, li, pos, rg)
        for li, pk in enumerate(layers):
            decoder_layer(self, dt, x, pk, li, proj=proj, qkv_to=qkv_to, attn=attn, rope=(cpos, spos), rope_seq=rs, fuse=fuse)
        if cache.lens is not None:
            cache.lens = [n + 1 for n in cache.lens]
        cache.len = pos + 1
        h16, h32 = hip.rmsnorm(x, self.norm.weight, cfg.rms_norm_eps, dtype=dt, want_f32=True)
        return h32.view(B, 1, D), h16

    def decode_attn(self, row, cache, li_, pos, rg=None):
        """the attention half of one decode layer, shared by the 16-bit, quantised-weight and LoRA steps (decode_step's `attn`).  row: the new tokens' fused [q | k | v] rows [B, 3D].
        Uniform (rg None): row IS row `pos` of the layer's cache buffer, every batch row attends keys [0, pos].  Ragged (rg: decode_step's per-step
        tables): row is the dense scratch — its [k | v] columns are scattered to position lens[b] of every cache row (one launch, kv_append_rows), then
        q is read from the scratch and row b attends its own lens[b] + 1 cached keys (the ragged decode kernels; fp32: stllm_attention's kv_len)."""
        B, D = row.shape[0], row.shape[1] // 3
        H = self.config.num_attention_heads
        hd = D // H
        if cache.base is not None:
            # shared base (rg: decode_step's tables in LOCAL positions): append to the cache's own rows, then every group of rows reads the base's P keys
            # once and each row its own suffix (bf16 / fp16: the shared-prefix decode kernels, 2 launches; fp32: the vector kernel).  No other kernel runs
            # in their place: an unsupported head_dim is an error of the C entry point
            hip.kv_append_rows(row, cache.qkv[li_], rg["pos"])
            (kp, vp, kp_strides), (ks, vs, ks_strides) = cache.base.kv(li_), cache.kv(li_)
            return hip.attention_shared(row[:, :D], kp, vp, ks, vs, B=B, G=cache.base.batch, H=H, Sq=1,
                                        P=cache.base_len, D=hd, scale=hd ** -0.5, max_sfx=rg["max_kv"], sfx_len=rg["kv_len"], q_strides=(3 * D, 3 * D),
                                        kp_strides=kp_strides, ks_strides=ks_strides)
        k, v, strides = cache.kv(li_)
        if rg is None:
            return hip.attention(row[:, :D], k, v, B=B, H=H, Sq=1, Skv=pos + 1, D=hd,
                                 scale=hd ** -0.5, causal=False, q_strides=strides, k_strides=strides, v_strides=strides)
        # the cache rows behind a row's length are UNINITIALISED memory.  The ragged decode kernels and the fp32 vector kernel bound their key loops by
        # kv_len and never read them; the 16-bit tile kernels load whole key tiles up to Skv and mask the scores only (0 x NaN would reach the output)
        if row.dtype != torch.float32 and (hd != 128 or not hip._decode_attn):
            raise NotImplementedError("ragged decode step in bf16 / fp16 needs the ragged decode attention kernels (head_dim 128, hip._decode_attn on)")
        hip.kv_append_rows(row, cache.qkv[li_], rg["pos"])
        return hip.attention(row[:, :D], k, v, B=B, H=H, Sq=1, Skv=rg["max_kv"], D=hd,
                             scale=hd ** -0.5, causal=False, kv_len=rg["kv_len"], q_strides=(3 * D, 3 * D), k_strides=strides, v_strides=strides)

    def new_cache(self, batch, max_len, device):
        return KVCache(len(self.layers), batch, max_len, self.config.hidden_size, runtime.compute_dtype(), device)

    def forward(self, input_ids=None, attention_mask=None, inputs_embeds=None, use_cache=False,
                output_hidden_states=False, return_dict=True, past_key_values=None, sp=None, **kw):
        if inputs_embeds is None:
            inputs_embeds = self.embed_tokens(input_ids)
        if sp is not None:   # this rank's position range of a sequence-parallel prefill (no cache: generate() prefills on one GPU)
            if use_cache or past_key_values is not None:
                raise NotImplementedError("sequence-parallel prefill does not fill a KV cache")
            hidden, h16, rows = self.prefill_sp(inputs_embeds, sp)
            out = Output(last_hidden_state=hidden, past_key_values=None, hidden_states=(hidden,) if output_hidden_states else None, attentions=None)
            out._h16, out._sp_rows = h16, rows
            return out
        if isinstance(past_key_values, KVCache) and past_key_values.base is not None:
            raise NotImplementedError("forward(past_key_values=) with a KV cache that has a shared base: use extend / decode_step, or fork() it")
        if isinstance(past_key_values, KVCache) and past_key_values.len > 0:   # decode step(s), one token at a time
            hs = []
            for t in range(inputs_embeds.shape[1]):
                hidden, h16 = self.decode_step(inputs_embeds[:, t:t + 1], past_key_values)
                hs.append(hidden)
            hidden = torch.cat(hs, dim=1) if len(hs) > 1 else hs[0]
            out = Output(last_hidden_state=hidden, past_key_values=past_key_values,
                         hidden_states=(hidden,) if output_hidden_states else None, attentions=None)
            out._h16 = h16
            return out
        cache = None
        if use_cache:
            cache = past_key_values if isinstance(past_key_values, KVCache) else \
                self.new_cache(inputs_embeds.shape[0], min(cfg_max_len(self.config), inputs_embeds.shape[1] + 512), inputs_embeds.device)
        hidden, h16 = self.prefill(inputs_embeds, attention_mask, cache=cache)
        out = Output(last_hidden_state=hidden, past_key_values=cache,
                     hidden_states=(hidden,) if output_hidden_states else None, attentions=None)
        out._h16 = h16
        return out


class LlamaForCausalLM(nn.Module):
    def __init__(self, config, device=None):
        super().__init__()
        self.config = config
        self.model = LlamaModel(config, device)
        self.vocab_size = config.vocab_size
        self.lm_head = Linear(config.hidden_size, config.vocab_size, bias=False, device=device)
        self._lm_packed = {}

    def lm_weight(self, dt):
        ver = (self.lm_head.weight._version, self.lm_head.weight.data_ptr(), runtime.gemm_split())
        hit = self._lm_packed.get(dt)
        if hit is None or hit[0] != ver:
            hit = (ver, pack.pad_rows(pack.linear(self.lm_head.weight, dt), 128))
            self._lm_packed = {dt: hit}
        return hit[1]

    def logits_from(self, h16, B, S):
        dt = runtime.compute_dtype()
        lg = hip.gemm(h16, self.lm_weight(dt), dtype=dt, out_f32=True)
        return lg.view(B, S, -1)[..., : self.vocab_size]
