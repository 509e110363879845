"""Caption generation on the native decoder: VALOR.generate_cap / decode_greedy / decode_beam / get_logits
(model/pretrain.py:914-1189), caption_type 'unimlm' | 'lm'.

The reference feeds [CLS] + generated tokens + [MASK] through the whole decoder again at every step (its cache path is disabled when the
decoder has cross-attention, pretrain.py:890-896, bert.py:848-850, and broken behind that, bert.py:807). Two things are cached here:

  * the video/audio K|V projections of the 12 layers are computed ONCE per clip (VALOR.cross_inputs) and shared by every step, every
    group and every beam;
  * the text rows' self-attention K|V (`DecodeSession`, SURVEY 8 row f4 "a working KV cache"). The generation mask is causal over the
    text and every text row sees the prompt rows, which see only themselves (bert.py:879-885): a position's hidden states never change
    once its token is fixed. A decoding step therefore runs TWO rows per sequence -- the token chosen by the previous step at
    position t and the [MASK] at t + 1 ('lm': one row) -- against per-layer K|V slots [prompt | text positions]; the prompt rows run
    once per clip. The step has static shapes and no host-built tensor (the step counter, the key-validity mask and the slot indices
    live on the device), so it is captured ONCE per geometry as a hipGraph and replayed: ~250 launches per step leave the host.
    Sessions (static buffers + graph) are kept per model and geometry and reused across batches and query groups.
    VALOR_KV_CACHE=0 selects the re-run-everything path (`_Stepper`, also the teacher-forced logits the parity tests use);
    VALOR_DECODE_GRAPH=0 runs the cached step eagerly.

There is ONE greedy, ONE beam and ONE sampled loop (`decode_greedy`, `decode_beam`, `decode_sample`), written against a step source:
  source.m                            the model (its .device)
  source.step(tok=None, parent=None)  fp32 logits [>= rows, V] with unit column stride of the step that follows the tokens `tok` (int64
                                      [rows] on the device; None: [CLS], the first step) on the sequences `parent` (int64 [rows]: beam
                                      search, row r continues row parent[r] of the previous step)
  source.poll                         every how many steps a loop asks (one host synchronisation) whether every row has ended
The sources are `DecodeSession` (poll 8: nothing else of a step waits for the device) and `_Rerun`, which keeps the tokens so far on the
host for a `_Stepper` (poll 1: it synchronises every step to fetch the tokens, and a step it need not run is a whole decoder).
Rows are beam-major everywhere (row = beam * b + sample), so that a row's cross-attention K|V is row % b -- the kv_bmod addressing the
training passes use -- instead of beam copies of K|V (pretrain.py:1133-1139 expands video_input / audio_input beam_size times); the
reference's (sample, beam) order is only that of the loop's own [b, beam, ...] bookkeeping.

Generation controls (`Constraints`: repetition penalty, no repeated n-gram, minimum length, suppressed tokens) are one
valor_logits_constrain launch per step on the step's logits, between the step and the selection, in every loop below; with the controls
off no launch is issued. `constrain_rows_host` restates the kernel's law on the host.

Closed answer sets (`AnswerSet`: a token trie of candidates, shared or one per sample): `candidates=` makes every loop decode INSIDE the
set with one valor_trie_constrain launch per step in the same place (`trie_rows_host` is its law on the host), and `score_candidates`
returns the exact sequence log-probability of every candidate by forced decoding through the same step sources. `rank_candidates` ranks
a whole shared set exactly, level by level over the trie: one decoder row per trie node, a node's logits row scoring all its children
(valor_trie_score_level; `trie_level_host` is its law on the host).

`decode_beam` restates the reference's beam rule (an ended beam stays in the beam). `decode_beam_pool` (beam_search='pool') is the search
with a pool of finished hypotheses: the beam stays `beam` OPEN hypotheses wide, length_penalty ranks while the search runs, the n best
are returned and the loop leaves early; one valor_beam_pool_step launch per step does the selection, the pool update, the history
reorder and the next step's inputs (`beam_pool_step_host` / `decode_beam_pool_host` are its law on the host, bit for bit).
`num_beam_groups` / `diversity_penalty` make it diverse beam search: the beam's groups are searched one after another inside ONE
valor_beam_group_step launch per step, a later group paying for every word an earlier group has just taken (`beam_group_step_host`).

Everything here is inference: torch.no_grad, dropout off regardless of model.training (the reference calls it under model.eval())."""
import contextlib
import gc
import os

import torch

from . import kernels as K, lib, ops
from .model.valor import PROMPTS, _BlockKV

BOS, EOS, MASK = 101, 102, 103          # [CLS] / [SEP] / [MASK] of bert-base-uncased, model/modeling.py:669-671


def _st():
    return K._stream()


class _Stepper:
    """get_logits + forward_cap_single(compute_loss=False), pretrain.py:1031-1051,882-900, for one query group."""

    def __init__(self, model, group, kv_layers, ranges, prompt_cpu, b):
        self.m, self.kv, self.b, self.prompt = model, kv_layers, b, prompt_cpu
        self.range = list(ranges[group]) if kv_layers is not None else None
        self.blocks = isinstance(kv_layers, _BlockKV)

    def logits(self, state, rows):
        """state: host int64 [rows, t], rows beam-major (None at t = 0) -> fp32 logits [rows, vocab] of the last text position:
        the appended [MASK] (caption_type 'unimlm') or the last token itself ('lm': [CLS] + the tokens so far, pretrain.py:1038-1040).
        full_masker does not reach this path in the reference either (forward_cap_single's generation branch, :878-900, drops the flag)."""
        m, b = self.m, self.b
        beam = rows // b
        bos = torch.full((rows, 1), BOS, dtype=torch.long)
        if m.caption_type == "lm":
            txt = bos if state is None else torch.cat((bos, state), dim=1)
        else:
            mask_col = torch.full((rows, 1), MASK, dtype=torch.long)
            txt = torch.cat((bos, mask_col), dim=1) if state is None else torch.cat((bos, state, mask_col), dim=1)
        prompt = None
        if self.prompt is not None:                                 # one prompt row per SAMPLE (a QA question differs per clip): beam-major copies
            prompt = self.prompt.repeat(beam, 1) if beam > 1 else self.prompt
        T = txt.shape[1]
        x = m._bert_embed(m._dev(txt), T, None)
        if prompt is not None:
            x = torch.cat((x, m._bert_embed(m._dev(prompt), prompt.shape[1], "prompt")), dim=1)
        Ttot = x.shape[1]
        amask = m._dev(m._bert_mask(txt, prompt, True))
        kv_range = None
        if self.blocks:                                             # a cross-attention block per modality: the group is a tuple of modalities
            kv_range = tuple(self.range)
        elif self.kv is not None:
            kv_range = m._dev(torch.tensor([self.range] * rows, dtype=torch.int32))
        hidden = m.bert_encoder(x, amask, self.kv, kv_range, b if self.kv is not None else 0)
        idx = m._dev(torch.arange(rows, dtype=torch.int64) * Ttot + (T - 1))
        h = m.cls_transform(ops.gather_rows(hidden.reshape(-1, hidden.shape[-1]), idx))
        P = m.P
        return K.gemm(h, P["multimodal_encoder.embeddings.word_embeddings.weight"], bias=P["cls.decoder.bias"], out_dtype=torch.float32)


class _Rerun:
    """A _Stepper as a step source: the tokens so far live on the host, [rows, t] beam-major, and every step runs all of them again.
    The first step runs b rows; a later one as many as `tok` has."""
    poll = 1

    def __init__(self, stepper):
        self.m, self.stepper, self.state = stepper.m, stepper, None

    def step(self, tok=None, parent=None):
        if tok is None:
            return self.stepper.logits(None, self.stepper.b)
        if parent is not None and self.state is not None:          # every sequence continues the row `parent` of the previous step
            self.state = self.state[parent.cpu()]
        w = tok.cpu().unsqueeze(1)
        self.state = w if self.state is None else torch.cat((self.state, w), dim=1)
        return self.stepper.logits(self.state, tok.numel())


NEG = -10000.0                           # the additive mask value of BertModel.forward (bert.py:885)


def kv_cache_enabled():
    return os.environ.get("VALOR_KV_CACHE", "1") != "0"


class DecodeSession:
    """Static buffers + the captured decoding step of one geometry: R = b * beam sequences, J new rows per step (2: token + [MASK],
    'unimlm'; 1: 'lm'), P prompt slots, `max_len` generated tokens, the per-layer [video | audio] K|V shape.

    Slots of a layer's self-attention K|V, per sequence: [0, P) the prompt rows (written once per clip by `begin_group`), P + i the
    text position i. Step t writes the token's K|V to slot P + t and the [MASK]'s to P + t + 1 (overwritten by the next step's token);
    `kmask` [R, L] holds 0 / -10000 per written slot (a key whose token id is 0 is masked, bert.py:857,885: prompt padding, and a
    generated id 0), the step's attention mask opens slots <= P + t for the token row and P + t + 1 besides for the [MASK] row.
    Rows are beam-major (row = beam * b + sample); a beam step first moves every sequence's slots to the row that continues it
    (`parent`)."""
    poll = 8                                           # a finished row keeps producing [SEP] (pretrain.py:1005-1010): asking late costs a few cheap steps

    def __init__(self, model, b, beam, P, max_len, kv_layers):
        m = self.m = model
        dev, dt, E = m.device, m.dtype, m.spec.hidden
        self.b, self.beam, self.R, self.P, self.max_len = b, beam, b * beam, P, max_len
        self.J = 1 if m.caption_type == "lm" else 2
        self.L = P + max_len + self.J - 1
        self.layers = m.spec.layers
        R, L, J = self.R, self.L, self.J
        i64 = dict(dtype=torch.int64, device=dev)
        # beam search: every sequence continues the row `parent` of the previous step -- two slot buffers, the step gathers the rows of the
        # one into the other with ONE launch of the row-gather kernel over all layers (a torch index_select + copy back was 0.42 of a 3.8 ms
        # step). VALOR_BEAM_TABLE=1: the slots never move (a token slot is written once and read-only afterwards), a [R, L] table of row
        # numbers follows the beams and the attention kernel reads slot j of sequence r from row slot_row[r, j]: half the slot memory, no
        # gather traffic -- and measured EQUAL (profiles/r06_generation_beam_table{,_off}.json: 553.9 vs 556.6 captions/s), so not the default.
        self.table = beam > 1 and os.environ.get("VALOR_BEAM_TABLE", "0") != "0"
        self.caches = [torch.zeros((self.layers, R, L, 2 * E), dtype=dt, device=dev) for _ in range(2 if beam > 1 and not self.table else 1)]
        self.rows32 = torch.arange(R, device=dev, dtype=torch.int32)
        self.slot_row = self.rows32[:, None].expand(R, L).contiguous() if self.table else None
        self.cache = self.caches[0]                    # the buffer that holds the sequences' slots now
        self.step_i = 0                                # steps of the current group so far (host side: which buffer is live)
        self.layer_base = (torch.arange(self.layers, device=dev, dtype=torch.int64) * R)[:, None]
        self.kmask = torch.full((R, L), NEG, dtype=torch.float32, device=dev)
        self.amask = torch.empty((R, J, L), dtype=torch.float32, device=dev)
        self.t = torch.zeros(1, **i64)
        self.tok = torch.full((R,), BOS, **i64)
        self.parent = torch.arange(R, **i64)
        self.ids = torch.full((R, J), MASK, **i64)
        self.slot = torch.arange(L, **i64)
        self.jidx = torch.arange(J, **i64)
        self.kv = None
        if kv_layers is not None:
            self.kv = [torch.empty_like(kv) for kv in kv_layers]
            self.cross_range = torch.zeros((R, 2), dtype=torch.int32, device=dev)
        self.graphs, self.logits_of, self.pool = {}, {}, None
        self.logits_pad = self.slots_buf = None
        self.fused_head = dev.type == "cuda" and os.environ.get("VALOR_DECODE_PROLOGUE", "1") != "0"
        self.eager_steps = 0
        self.use_graph = dev.type == "cuda" and os.environ.get("VALOR_DECODE_GRAPH", "1") != "0"

    @staticmethod
    def key(model, b, beam, P, max_len, kv_layers):
        kvs = None if kv_layers is None else (tuple(kv_layers[0].shape), len(kv_layers))
        return (b, beam, P, max_len, kvs, model.caption_type)

    def begin_batch(self, kv_layers):
        """the clips' per-layer [video | audio] K|V into the session's static buffers (once per batch: every group reads them)"""
        if kv_layers is not None:
            for dst, src in zip(self.kv, kv_layers):
                dst.copy_(src)

    def begin_group(self, key_range, prompt_cpu):
        """reset the text slots; run the prompt rows (one set per clip, bert.py:879-885: they attend to themselves only) and keep their
        per-layer K|V in slots [0, P) of every beam's row"""
        m, b, P, E = self.m, self.b, self.P, self.m.spec.hidden
        self.step_i, self.cache = 0, self.caches[0]
        self.t.zero_()
        self.tok.fill_(BOS)
        self.parent.copy_(self.layer_base.new_tensor(range(self.R)))
        if self.table:
            self.slot_row.copy_(self.rows32[:, None].expand(self.R, self.L))
        self.kmask.fill_(NEG)
        if self.kv is not None:
            self.cross_range.copy_(m._dev(torch.tensor([list(key_range)] * self.R, dtype=torch.int32)))
        if P:
            valid = m._dev((prompt_cpu != 0).to(torch.float32))                                 # [b, P]
            pm = (1.0 - valid) * NEG
            self.kmask.view(self.beam, b, self.L)[:, :, :P] = pm[None]
            pmask = pm[:, None, :].expand(b, P, P).contiguous()
            xp = m._bert_embed(m._dev(prompt_cpu), P, "prompt")
            cache = self.cache.view(self.layers, self.beam, b, self.L, 2 * E)

            def prefill(i, qkv):
                cache[i, :, :, :P] = qkv[:, :, E:][None]
                return ops.self_attention(qkv, m.spec.heads, pmask, 0.0)
            m.bert_encoder(xp, pmask, self.kv, self.cross_range[:b] if self.kv is not None else None, b if self.kv is not None else 0,
                           self_attn=prefill)

    # ------------------------------------------------------------------ one decoding step (eager, and what the graph captures)
    def _self_attn(self, i, qkv):
        E, c = self.m.spec.hidden, self.cache[i]
        c.index_copy_(1, self.slots_new, qkv[:, :, E:])
        if self.table:
            return K.attn_decode(qkv[:, :, :E], c[:, :, :E], c[:, :, E:], self.m.spec.heads, mask=self.amask, key_row=self.slot_row, scale=0.125)
        o, _ = K.attn_fwd(qkv[:, :, :E], c[:, :, :E], c[:, :, E:], self.m.spec.heads, mask=self.amask, scale=0.125)
        return o

    def _body(self, cur=0):
        """cur: which of the two slot buffers holds the sequences' state when the step starts (beam search; greedy has one)"""
        m, P_, J = self.m, self.m.P, self.J
        e = "multimodal_encoder.embeddings."
        self.cache = self.caches[cur]
        if self.table:                                              # every sequence continues the row `parent` of the previous step
            self.slot_row.copy_(self.slot_row.index_select(0, self.parent))
            self.kmask.copy_(self.kmask.index_select(0, self.parent))
        elif self.beam > 1:
            src, dst = self.caches[cur], self.caches[1 - cur]
            idx = (self.layer_base + self.parent[None, :]).reshape(-1)
            words = src[0, 0].numel() * src.element_size() // 4      # a sequence's slots of one layer as 32-bit words (16-byte accesses)
            lib.call("valor_gather_rows", _st(), lib.DT_F32, src.data_ptr(), idx.data_ptr(), dst.data_ptr(), idx.numel(), words, words)
            self.kmask.copy_(self.kmask.index_select(0, self.parent))
            self.cache = dst
        Wd, Pe, Ty = P_[e + "word_embeddings.weight"], P_[e + "position_embeddings.weight"], P_[e + "token_type_embeddings.weight"]
        if self.fused_head and Wd.dtype == Pe.dtype == Ty.dtype == m.dtype and Wd.is_contiguous() and Pe.is_contiguous() and Ty.is_contiguous():
            # embeddings before their LayerNorm, the step's mask rows, its slots: one launch (valor_decode_prologue) for the ~22 below
            x = torch.empty((self.R, J, Wd.shape[1]), dtype=m.dtype, device=Wd.device)
            if self.slots_buf is None:
                self.slots_buf = torch.zeros(J, dtype=torch.int64, device=Wd.device)
            lib.call("valor_decode_prologue", _st(), K.dt_of(x), self.tok.data_ptr(), self.t.data_ptr(), Wd.data_ptr(), Pe.data_ptr(), Ty.data_ptr(),
                     MASK, self.R, J, Wd.shape[1], self.P, self.L, NEG, self.kmask.data_ptr(), self.amask.data_ptr(), x.data_ptr(),
                     self.slots_buf.data_ptr())
            self.slots_new = self.slots_buf
            if self.table:
                self.slot_row.index_copy_(1, self.slots_new, self.rows32[:, None].expand(self.R, J).contiguous())
            x = ops.layer_norm(x, P_[e + "LayerNorm.weight"], P_[e + "LayerNorm.bias"], 1e-12)
            return self._tail(x)
        self.ids[:, 0] = self.tok
        pos = self.t + self.jidx
        # BertEmbeddings (bert.py:190-218) at positions t, t + 1: the embedding kernel's arithmetic (fp32 sum, one rounding)
        x = (P_[e + "word_embeddings.weight"][self.ids].float() + P_[e + "position_embeddings.weight"][pos].float()[None]
             + P_[e + "token_type_embeddings.weight"][0].float()).to(m.dtype)
        x = ops.layer_norm(x, P_[e + "LayerNorm.weight"], P_[e + "LayerNorm.bias"], 1e-12)
        slot_t = self.t + self.P
        self.kmask.index_copy_(1, slot_t, torch.where(self.tok != 0, 0.0, NEG)[:, None])
        row_a = torch.where(self.slot <= slot_t, self.kmask, NEG)
        self.amask[:, 0] = row_a
        if J == 2:
            self.amask[:, 1] = torch.where(self.slot == slot_t + 1, 0.0, row_a)
        self.slots_new = slot_t + self.jidx
        if self.table:                                              # this step's slots are the row's own
            self.slot_row.index_copy_(1, self.slots_new, self.rows32[:, None].expand(self.R, J).contiguous())
        return self._tail(x)

    def _tail(self, x):
        m, P_, J = self.m, self.m.P, self.J
        e = "multimodal_encoder.embeddings."
        hidden = m.bert_encoder(x, None, self.kv, self.cross_range if self.kv is not None else None, self.b if self.kv is not None else 0,
                                self_attn=self._self_attn)
        h = m.cls_transform(hidden[:, J - 1].contiguous())
        if self.logits_pad is None:                                   # rows of a zero-padded static buffer (first, eager, step of the session):
            V = P_[e + "word_embeddings.weight"].shape[0]             # log_softmax_rows reads them in place
            self.logits_pad = torch.zeros((h.shape[0], (V + 31) // 32 * 32), dtype=torch.float32, device=h.device)[:, :V]
        logits = self.logits_pad
        K.gemm(h, P_[e + "word_embeddings.weight"], bias=P_["cls.decoder.bias"], out=logits, out_dtype=torch.float32, policy=K.infer_policy())
        self.t += 1
        return logits

    def _capture(self, cur):
        from . import graphs
        dev = self.m.device
        ctx = graphs._capture_ctx(dev)
        with torch.cuda.stream(ctx["stream"]):         # the capture stream's kernel scratch must not come out of the graph's pool
            K.workspace(dev)
            K.ReduceQueue.current(dev)
        if self.pool is None:
            self.pool = torch.cuda.graph_pool_handle()
        g = torch.cuda.CUDAGraph()
        mode = "thread_local" if (torch.distributed.is_available() and torch.distributed.is_initialized()) else "global"
        torch.cuda.current_stream(dev).synchronize()
        with no_gc(), torch.cuda.graph(g, pool=self.pool, stream=ctx["stream"], capture_error_mode=mode):
            self.logits_of[cur] = self._body(cur)
        self.graphs[cur] = g

    def step(self, tok=None, parent=None):
        """tok int64 [R] (device; None: [CLS], the first step), parent int64 [R] (beam search) -> fp32 logits [R, vocab] of the step's
        last row (a static buffer when the step is a graph replay: consume it before the next step)"""
        if tok is not None:
            self.tok.copy_(tok)
        if parent is not None:
            self.parent.copy_(parent)
        cur = self.step_i % len(self.caches)
        self.step_i += 1
        if cur not in self.graphs:
            if not self.use_graph or self.eager_steps < 1:
                self.eager_steps += 1
                return self._body(cur)
            self._capture(cur)
        self.graphs[cur].replay()
        self.cache = self.caches[(1 - cur) % len(self.caches)]
        return self.logits_of[cur]


MAX_SESSIONS = 4


def session(model, b, beam, P, max_len, kv_layers):
    """the model's DecodeSession of this geometry (most recently used last; at most MAX_SESSIONS are kept)"""
    pool = model.__dict__.setdefault("_decode_sessions", {})
    key = DecodeSession.key(model, b, beam, P, max_len, kv_layers)
    s = pool.pop(key, None)
    if s is None:
        while len(pool) >= MAX_SESSIONS:
            pool.pop(next(iter(pool)))
        s = DecodeSession(model, b, beam, P, max_len, kv_layers)
    pool[key] = s
    return s


def release_sessions(model):
    """drop the decoding sessions (their K|V slots, the copies of the clips' K|V and the captured graphs)"""
    model.__dict__.pop("_decode_sessions", None)


def _xent_rows(logits, labels=None):
    """valor_xent_fwd on fp32 rows -> (row loss lse(z) - z[label], lse, the zero-padded buffer the rows sit in); labels None: column 0"""
    n, V = logits.shape
    Vpad = (V + 31) // 32 * 32
    if logits.stride() == (Vpad, 1) and logits.data_ptr() % 16 == 0:       # the decoding session's rows already sit in a zero-padded buffer
        buf = logits
    else:
        buf = torch.zeros((n, Vpad), dtype=torch.float32, device=logits.device)
        buf[:, :V] = logits
    lse = torch.empty(n, dtype=torch.float32, device=logits.device)
    loss = torch.empty(n, dtype=torch.float32, device=logits.device)
    if labels is None:
        labels = torch.zeros(n, dtype=torch.int64, device=logits.device)
    lib.call("valor_xent_fwd", _st(), lib.DT_F32, buf.data_ptr(), labels.data_ptr(), loss.data_ptr(), lse.data_ptr(), n, V, Vpad)
    return loss, lse, buf


def row_lse(logits):
    """log-sum-exp of fp32 rows (the cross-entropy kernel's) and the zero-padded buffer the rows sit in"""
    return _xent_rows(logits)[1:]


def log_softmax_rows(logits):
    """F.log_softmax(logits, dim=1) of fp32 rows (pretrain.py:1078): the row log-sum-exp comes from the cross-entropy kernel."""
    return logits - row_lse(logits)[0][:, None]


def beam_select_enabled():
    return os.environ.get("VALOR_BEAM_SELECT", "1") != "0"


def beam_select(logits, b, cur, beam, seq_logprob, seq_mask, beam_major, lse="kernel", lse_out=None, lse_rows=None):
    """candidate scores + `select` (pretrain.py:1080-1098,1156-1159) in one launch (valor_beam_select): logits fp32 [b * cur, V], rows
    beam-major (row = k * b + s) or sample-major; seq_logprob [b, cur | 1, 1], seq_mask [b, cur, 1] (1: open) -> (values, indices) [b, beam].
    lse: 'kernel' (the rows' log-sum-exp inside the launch; left in lse_out [b * cur] if given) or 'xent' (the cross-entropy kernel's);
    lse_rows fp32 [b * cur]: the rows' log-sum-exp computed by the caller (decoding inside an answer set: the row BEFORE its mask)"""
    V = logits.shape[1]
    dev = logits.device
    if lse_rows is not None:
        lse_t, buf = lse_rows, (logits if logits.stride(1) == 1 else logits.contiguous())
    elif lse == "xent":
        lse_t, buf = row_lse(logits)
    else:
        lse_t, buf = None, (logits if logits.stride(1) == 1 else logits.contiguous())
    sl = seq_logprob.reshape(b, -1).expand(b, cur).contiguous()
    sm = seq_mask.reshape(b, -1)[:, :cur].contiguous()
    val = torch.empty((b, beam), dtype=torch.float32, device=dev)
    idx = torch.empty((b, beam), dtype=torch.int64, device=dev)
    rs_s, rs_k = (1, b) if beam_major else (cur, 1)
    lib.call("valor_beam_select", _st(), buf.data_ptr(), buf.stride(0), rs_s, rs_k, None if lse_t is None else lse_t.data_ptr(), sl.data_ptr(),
             sm.data_ptr(), b, cur, V, beam, val.data_ptr(), idx.data_ptr(), None if lse_out is None else lse_out.data_ptr())
    return val, idx


class Constraints:
    """the controls of a generation, applied to every step's logits before the selection (valor_logits_constrain, one launch per step):
    repetition_penalty (1: off; the logit of every token generated so far is divided by it when positive, multiplied when not),
    no_repeat_ngram_size (0: off; no n-gram occurs twice in a sequence), min_length (no [SEP] before that many tokens),
    suppress_tokens (ids that are never generated). length_penalty = alpha (0: off) belongs to beam search alone: the final pick among
    the `beam` hypotheses ranks them by logP / length^alpha. The defaults are all off: the decoders of the reference."""
    __slots__ = ("repetition_penalty", "no_repeat_ngram_size", "min_length", "suppress_tokens", "length_penalty")

    def __init__(self, repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, suppress_tokens=(), length_penalty=0.0):
        repetition_penalty, length_penalty = float(repetition_penalty), float(length_penalty)
        if not (repetition_penalty > 0.0 and repetition_penalty != float("inf")):
            raise ValueError(f"Constraints: repetition_penalty {repetition_penalty!r} must be a finite number > 0 (1: off)")
        if float(torch.tensor(repetition_penalty, dtype=torch.float32)) in (0.0, float("inf")):
            raise ValueError(f"Constraints: repetition_penalty {repetition_penalty!r} is not a finite fp32 number > 0")
        if int(no_repeat_ngram_size) != no_repeat_ngram_size or no_repeat_ngram_size < 0:
            raise ValueError(f"Constraints: no_repeat_ngram_size {no_repeat_ngram_size!r} must be an integer >= 0 (0: off)")
        if int(min_length) != min_length or min_length < 0:
            raise ValueError(f"Constraints: min_length {min_length!r} must be an integer >= 0")
        if suppress_tokens is None:
            suppress_tokens = ()
        if torch.is_tensor(suppress_tokens):
            suppress_tokens = suppress_tokens.reshape(-1).tolist()
        for w in suppress_tokens:
            if int(w) != w or not (-2 ** 31 <= w < 2 ** 31):
                raise ValueError(f"Constraints: suppress_tokens holds {w!r}: token ids are 32-bit integers")
        if length_penalty != length_penalty or length_penalty in (float("inf"), -float("inf")):
            raise ValueError(f"Constraints: length_penalty {length_penalty!r} must be a finite number (0: off)")
        self.repetition_penalty, self.no_repeat_ngram_size, self.min_length = repetition_penalty, int(no_repeat_ngram_size), int(min_length)
        self.suppress_tokens, self.length_penalty = tuple(int(w) for w in suppress_tokens), length_penalty

    @property
    def logits_off(self):
        """no rule of valor_logits_constrain is on: no launch"""
        return self.repetition_penalty == 1.0 and self.no_repeat_ngram_size == 0 and self.min_length == 0 and not self.suppress_tokens

    @property
    def off(self):
        return self.logits_off and self.length_penalty == 0.0

    @property
    def penalty(self):
        """repetition_penalty rounded to fp32: what the kernel multiplies by"""
        return float(torch.tensor(self.repetition_penalty, dtype=torch.float32))

    @property
    def inv_penalty(self):
        """1 / repetition_penalty rounded to fp32: the kernel's other factor"""
        return float(torch.tensor(1.0 / self.repetition_penalty, dtype=torch.float32))

    def __repr__(self):
        return (f"Constraints(repetition_penalty={self.repetition_penalty}, no_repeat_ngram_size={self.no_repeat_ngram_size}, "
                f"min_length={self.min_length}, suppress_tokens={self.suppress_tokens}, length_penalty={self.length_penalty})")


def constrain_rows_host(logits, hist, t, constraints, eos, active=None):
    """Rules 1-4 of valor_logits_constrain (include/valor_hip.h) restated on the host in fp32: logits [R, V] (any device; not modified),
    hist int64 [R, >= t] in ROW order (row r's own tokens; None while t == 0), active [R] or None -> a new fp32 host tensor [R, V].
    A single fp32 multiply per penalised column and -inf writes: bit-identical to the kernel."""
    c = constraints
    out = logits.detach().to(device="cpu", dtype=torch.float32).clone()
    R, V = out.shape
    pen, inv = torch.tensor(c.penalty, dtype=torch.float32), torch.tensor(c.inv_penalty, dtype=torch.float32)
    n = c.no_repeat_ngram_size
    ninf = -float("inf")
    for r in range(R):
        if active is not None and not bool(active[r]):
            continue
        h = [] if t == 0 else hist[r, :t].tolist()
        z = out[r]
        if c.penalty != 1.0:
            seen = sorted({w for w in h if 0 <= w < V})
            if seen:
                idx = torch.tensor(seen, dtype=torch.long)
                x = z[idx]
                z[idx] = torch.where(x > 0, x * inv, x * pen)
        if n >= 1 and t >= n - 1:
            tail = h[t - n + 1:]
            for i in range(t - n + 1):
                if h[i:i + n - 1] == tail and 0 <= h[i + n - 1] < V:
                    z[h[i + n - 1]] = ninf
        if t < c.min_length:
            z[eos] = ninf
        for w in c.suppress_tokens:
            if 0 <= w < V:
                z[w] = ninf
    return out


class _Constrainer:
    """the per-step launch of a decode loop under `constraints`: holds the device copy of the suppress list"""

    def __init__(self, constraints, dev):
        c = self.c = constraints
        self.penalty, self.inv_penalty = c.penalty, c.inv_penalty
        self.suppress = torch.tensor(c.suppress_tokens, dtype=torch.int32, device=dev) if c.suppress_tokens else None

    def __call__(self, logits, hist, t, active, b=None, hist_stride_s=None, hist_stride_k=0):
        c = self.c
        return K.logits_constrain(logits, hist if t > 0 else None, t, EOS, self.penalty, self.inv_penalty, c.no_repeat_ngram_size, c.min_length,
                                  self.suppress, active, b, hist_stride_s, hist_stride_k)


def _constrainer(constraints, dev, candidates=None):
    """None when no rule touches the logits: the loops then issue no launch and are the parent's, bit for bit. candidates: an AnswerSet
    -> the launch is valor_trie_constrain (never both: _check_candidates)"""
    if candidates is not None:
        _no_logits_rules(constraints)
        return _TrieConstrainer(candidates, dev)
    return None if constraints is None or constraints.logits_off else _Constrainer(constraints, dev)


def _no_logits_rules(constraints):
    if constraints is not None and not constraints.logits_off:
        raise ValueError("candidates= together with a logits rule of Constraints (repetition_penalty / no_repeat_ngram_size / min_length "
                         "/ suppress_tokens) can leave a row without an allowed token; only length_penalty combines with an answer set")


TRIE_FLOOR = lib.TRIE_FLOOR              # VALOR_TRIE_FLOOR of include/valor_hip.h


class AnswerSet:
    """A closed set of answers as a token trie, for decoding inside it (valor_trie_constrain) and for looking answers up (index_of).
    candidates: a list of token-id lists without [CLS] / [SEP] (per_sample=False: one set for every row), or a list with one such list
    per decoder row-sample (per_sample=True). Duplicates are allowed; the lowest index names the answer. vocab: the vocabulary size the
    ids are checked against (None: checked when the set meets a model, check_vocab).
    The trie, flattened to CSR (host int32 / uint8 tensors; .device(dev) caches a device copy): child_ptr [N + 1], child_tok [E]
    ascending inside a node, child_node [E], terminal [N], root [n_roots] (n_roots = 1, or one root per sample)."""

    def __init__(self, candidates, per_sample=False, vocab=None):
        sets = [list(s) for s in candidates] if per_sample else [list(candidates)]
        if not sets:
            raise ValueError("AnswerSet: no sample")
        self.per_sample = bool(per_sample)
        kids, term, first = [], [], []                  # per node: {token: node}, a candidate ends here, the lowest index that does

        def new():
            kids.append({}); term.append(0); first.append(-1)
            return len(kids) - 1
        roots, self.counts, self.max_len = [], [], 0
        self.candidates = []
        for s, cands in enumerate(sets):
            where = f" of sample {s}" if per_sample else ""
            if not cands:
                raise ValueError(f"AnswerSet: the set{where} is empty")
            root = new()
            roots.append(root)
            rows = []
            for ci, cand in enumerate(cands):
                cand = cand.tolist() if torch.is_tensor(cand) else list(cand)
                if not cand:
                    raise ValueError(f"AnswerSet: candidate {ci}{where} is empty")
                node = root
                for w in cand:
                    if int(w) != w or w < 1 or w == EOS or (vocab is not None and w >= vocab):
                        raise ValueError(f"AnswerSet: candidate {ci}{where} holds id {w!r}: ids lie in [1, V) and are not [SEP] = {EOS} "
                                         "(id 0 is a masked key in this decoder)")
                    w = int(w)
                    nxt = kids[node].get(w)
                    if nxt is None:
                        nxt = kids[node][w] = new()
                    node = nxt
                if not term[node]:
                    term[node], first[node] = 1, ci
                rows.append([int(w) for w in cand])
                self.max_len = max(self.max_len, len(cand))
            self.candidates.append(rows)
            self.counts.append(len(rows))
        ptr, tok, nod = [0], [], []
        for k in kids:
            for w in sorted(k):
                tok.append(w); nod.append(k[w])
            ptr.append(len(tok))
        self.child_ptr = torch.tensor(ptr, dtype=torch.int32)
        self.child_tok = torch.tensor(tok, dtype=torch.int32)
        self.child_node = torch.tensor(nod, dtype=torch.int32)
        self.terminal = torch.tensor(term, dtype=torch.uint8)
        self.root = torch.tensor(roots, dtype=torch.int32)
        self.first = first
        self.vocab = vocab
        self._kids = kids
        self._dev = {}

    @classmethod
    def from_bert_rows(cls, rows, per_sample_counts=None, vocab=None):
        """rows: int [n, T] of '[CLS] tokens [SEP] 0...' (choice_tokens['bert_tokens']) -> the set of the n answers, or with
        per_sample_counts = [c_0, c_1, ..] a per-sample set: the first c_0 rows belong to sample 0, the next c_1 to sample 1, ..."""
        rows = rows.tolist() if torch.is_tensor(rows) else [list(r) for r in rows]
        cands = []
        for i, r in enumerate(rows):
            if not r or r[0] != BOS or EOS not in r:
                raise ValueError(f"AnswerSet.from_bert_rows: row {i} is not '[CLS] tokens [SEP]'")
            cands.append(r[1:r.index(EOS)])
        if per_sample_counts is None:
            return cls(cands, vocab=vocab)
        counts = [int(c) for c in per_sample_counts]
        if sum(counts) != len(cands) or any(c < 0 for c in counts):
            raise ValueError(f"AnswerSet.from_bert_rows: per_sample_counts {counts} do not describe {len(cands)} rows")
        start = [sum(counts[:i]) for i in range(len(counts))]
        return cls([cands[s:s + c] for s, c in zip(start, counts)], per_sample=True, vocab=vocab)

    @property
    def n_roots(self):
        return int(self.root.numel())

    @property
    def n_nodes(self):
        return int(self.terminal.numel())

    def check_vocab(self, V):
        if self.child_tok.numel() and int(self.child_tok.max()) >= V:
            raise ValueError(f"AnswerSet: id {int(self.child_tok.max())} is outside the vocabulary [1, {V})")

    def device(self, dev):
        """the trie's arrays on `dev` (cached per device): what kernels.trie_constrain takes"""
        import types
        dev = torch.device(dev)
        d = self._dev.get(dev)
        if d is None:
            d = self._dev[dev] = types.SimpleNamespace(**{k: getattr(self, k).to(dev) for k in
                                                         ("child_ptr", "child_tok", "child_node", "terminal", "root")})
        return d

    def levels(self, dev=None):
        """the trie of a shared set in breadth-first order, for the level-batched exact ranking (`rank_candidates`): host tensors, cached
        on the set; with `dev` their copy on that device, cached like .device(dev).
          order int32 [N]: the node ids, level by level (level 0 = the root alone, parents before children, a node's children in
          ascending token order); level_ptr (a list, depth_max + 2 entries): level d = order[level_ptr[d] : level_ptr[d + 1]];
          depth / token / parent int32 [N], indexed by node id (the root: depth 0, token [CLS], parent -1);
          anc int32 [N, depth_max + 1]: anc[n, j] = the ancestor of n at depth j (j = depth[n]: n itself; deeper: -1);
          cand_node int64 [C]: the node where candidate c ends (duplicates share it); depth_max = the longest answer; width = the
          widest level."""
        import types
        if self.per_sample:
            raise ValueError("AnswerSet.levels: a per-sample set has one trie per sample; the level plan is that of a shared set")
        lv = self.__dict__.get("_levels")
        if lv is None:
            N = self.n_nodes
            ptr, tok, nod = self.child_ptr.tolist(), self.child_tok.tolist(), self.child_node.tolist()
            depth, token, parent = [0] * N, [BOS] * N, [-1] * N
            order, level_ptr, level = [], [0], [int(self.root[0])]
            while level:
                order += level
                level_ptr.append(len(order))
                nxt = []
                for n in level:
                    for e in range(ptr[n], ptr[n + 1]):
                        c = nod[e]
                        depth[c], token[c], parent[c] = depth[n] + 1, tok[e], n
                        nxt.append(c)
                level = nxt
            D = len(level_ptr) - 2
            anc = [[-1] * (D + 1) for _ in range(N)]
            for n in order:                                              # parents first: a node's row is its parent's plus itself
                if parent[n] >= 0:
                    anc[n][:depth[n]] = anc[parent[n]][:depth[n]]
                anc[n][depth[n]] = n
            cand_node = []
            for cand in self.candidates[0]:
                n = int(self.root[0])
                for w in cand:
                    n = self._kids[n][w]
                cand_node.append(n)
            i32 = lambda x: torch.tensor(x, dtype=torch.int32)
            lv = self._levels = types.SimpleNamespace(
                order=i32(order), level_ptr=level_ptr, depth=i32(depth), token=i32(token), parent=i32(parent), anc=i32(anc),
                cand_node=torch.tensor(cand_node, dtype=torch.int64), depth_max=D,
                width=max(level_ptr[d + 1] - level_ptr[d] for d in range(D + 1)))
            self._levels_dev = {}
        if dev is None:
            return lv
        dev = torch.device(dev)
        d = self._levels_dev.get(dev)
        if d is None:
            d = self._levels_dev[dev] = types.SimpleNamespace(**{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in vars(lv).items()})
        return d

    def with_roots(self, samples):
        """the same trie read by other rows: row-sample i of the result is sample samples[i] of this per-sample set (several question
        rows per clip, num_return_sequences)"""
        import copy
        out = copy.copy(self)
        idx = torch.as_tensor(samples, dtype=torch.long)
        out.root = self.root[idx].contiguous()
        out.counts = [self.counts[i] for i in idx.tolist()]
        out.candidates = [self.candidates[i] for i in idx.tolist()]
        out._dev = {}
        return out

    def for_rows(self, b, groups=None):
        """this set for b decoder row-samples: a shared set serves any b; a per-sample set of n entries serves b = n, or b = sum(groups)
        with len(groups) = n (entry i is read by groups[i] consecutive rows), or b = n * k (k consecutive rows per entry)"""
        n = self.n_roots
        if not self.per_sample or n == b:
            return self
        if groups is not None and len(groups) == n and sum(groups) == b:
            return self.with_roots([i for i, k in enumerate(groups) for _ in range(k)])
        if b % n == 0 and groups is None:
            return self.with_roots([i for i in range(n) for _ in range(b // n)])
        raise ValueError(f"AnswerSet: a per-sample set of {n} entries does not describe {b} decoder rows")

    def _step(self, node, w):
        """the child of `node` along token w, or -1 (the host's dictionaries: the same edges as the CSR arrays)"""
        return -1 if node < 0 else self._kids[node].get(int(w), -1)

    def index_of(self, seqs):
        """seqs int [R, L] (any device), every row cut at its first [SEP] (none: the whole row) -> int64 [R] (host): the candidate
        index of the row (the lowest among duplicates), -1 when the row is no candidate. Row r reads sample r % n_roots."""
        rows = seqs.tolist() if torch.is_tensor(seqs) else [list(r) for r in seqs]
        out = []
        for r, row in enumerate(rows):
            if EOS in row:
                row = row[:row.index(EOS)]
            node = int(self.root[r % self.n_roots])
            for w in row:
                node = self._step(node, w)
            out.append(self.first[node] if node >= 0 and row else -1)
        return torch.tensor(out, dtype=torch.int64)


def _answer_set(candidates):
    """candidates= of the generate_* calls: an AnswerSet, or a plain list of token lists (one shared set)"""
    if candidates is None or isinstance(candidates, AnswerSet):
        return candidates
    return AnswerSet(candidates)


def trie_rows_host(logits, hist, t, answer_set, eos, b, active=None):
    """The law of valor_trie_constrain (include/valor_hip.h) restated on the host from the CSR arrays: logits [R, V] (any device; not
    modified), hist int64 [R, >= t] in ROW order (row r's own tokens; None while t == 0), b: row r reads root r % b of a per-sample
    set, active [R] or None -> a new fp32 host tensor [R, V]. Only floor writes: bit-identical to the kernel."""
    a = answer_set
    out = logits.detach().to(device="cpu", dtype=torch.float32).clone()
    R, V = out.shape
    ptr, tok, nod, term, root = (x.tolist() for x in (a.child_ptr, a.child_tok, a.child_node, a.terminal, a.root))
    N, E = len(term), len(tok)
    if len(root) not in (1, b):
        raise ValueError(f"trie_rows_host: {len(root)} roots for b = {b}")
    floor = torch.tensor(TRIE_FLOOR, dtype=torch.float32)
    for r in range(R):
        if active is not None and not bool(active[r]):
            continue
        node = root[0 if len(root) == 1 else r % b]
        if not 0 <= node < N:
            node = -1
        for w in ([] if t == 0 else hist[r, :t].tolist()):
            if node < 0:
                break
            lo = min(max(ptr[node], 0), E)
            hi = min(max(ptr[node + 1], lo), E)
            nxt = -1
            for e in range(lo, hi):
                if tok[e] == w:
                    nxt = nod[e]
                    break
            node = nxt if 0 <= nxt < N else -1
        allowed = set()
        if node >= 0:
            lo = min(max(ptr[node], 0), E)
            allowed = {w for w in tok[lo:min(max(ptr[node + 1], lo), E)] if 0 <= w < V}
        if node < 0 or term[node]:
            allowed.add(int(eos))
        keep = torch.zeros(V, dtype=torch.bool)
        keep[torch.tensor(sorted(allowed), dtype=torch.long)] = True
        out[r] = torch.where(keep, out[r], floor)
    return out


def trie_level_host(logits, lse, level_node, b, answer_set, eos, node_score, final):
    """The law of valor_trie_score_level (include/valor_hip.h) restated on the host from the CSR arrays: logits [n_level * b, V] (any
    device; row i * b + s = node level_node[i], sample s), lse fp32 [rows] (the rows' log-sum-exp as the caller has it; None: torch's,
    which is not the kernel's bit for bit), node_score / final fp32 [n_nodes * b] (not modified) -> new host tensors (node_score,
    final). fp32 throughout, the subtraction rounded before the addition: bit-identical to the kernel for the same lse."""
    a = answer_set
    z = logits.detach().to(device="cpu", dtype=torch.float32)
    rows, V = z.shape
    ptr, tok, nod, term = (x.tolist() for x in (a.child_ptr, a.child_tok, a.child_node, a.terminal))
    N, E = len(term), len(tok)
    nodes = level_node.tolist() if torch.is_tensor(level_node) else list(level_node)
    if b < 1 or rows != len(nodes) * b:
        raise ValueError(f"trie_level_host: {rows} rows for {len(nodes)} nodes x b = {b}")
    l = torch.logsumexp(z, 1) if lse is None else lse.detach().to(device="cpu", dtype=torch.float32)
    ns = node_score.detach().to(device="cpu", dtype=torch.float32).clone().view(N, b)
    fin = final.detach().to(device="cpu", dtype=torch.float32).clone().view(N, b)
    for i, node in enumerate(nodes):
        if not 0 <= node < N:
            continue
        zr, lr, own = z[i * b:(i + 1) * b], l[i * b:(i + 1) * b], ns[node].clone()
        lo = min(max(ptr[node], 0), E)
        hi = min(max(ptr[node + 1], lo), E)
        edges = [e for e in range(lo, hi) if 0 <= tok[e] < V and 0 <= nod[e] < N]
        if edges:
            cols = torch.tensor([tok[e] for e in edges], dtype=torch.long)
            kids = torch.tensor([nod[e] for e in edges], dtype=torch.long)
            ns[kids] = own[None, :] + (zr[:, cols].t() - lr[None, :])
        if term[node]:
            fin[node] = own + (zr[:, int(eos)] - lr)
    return ns.reshape(-1), fin.reshape(-1)


class _TrieConstrainer:
    """the per-step valor_trie_constrain launch of a decode loop inside an AnswerSet: _Constrainer's call"""

    def __init__(self, answer_set, dev):
        self.trie = answer_set.device(dev)

    def __call__(self, logits, hist, t, active, b=None, hist_stride_s=None, hist_stride_k=0):
        return K.trie_constrain(logits, hist if t > 0 else None, t, EOS, self.trie, active, b, hist_stride_s, hist_stride_k)


def _check_candidates(model, candidates, constraints, max_len):
    """the AnswerSet of a generate_* call, or None; raises where the combination cannot work (for_rows(b) then fits it to the rows)"""
    a = _answer_set(candidates)
    if a is None:
        return None
    _no_logits_rules(constraints)
    if a.max_len > max_len - 1:
        raise ValueError(f"candidates: the longest answer has {a.max_len} tokens; with its [SEP] it does not fit in max_generation_len - 1 = "
                         f"{max_len - 1} tokens")
    a.check_vocab(model.spec.vocab)
    return a


def _final_beam_order(seq_logprob, outputs, max_len, constraints):
    """the final ranking of the `beam` hypotheses: seq_logprob [b, beam, 1], outputs int64 [b, beam, max_len] -> sort_idx [b, beam, 1].
    length_penalty alpha == 0: the reference's sort of the summed logP. Otherwise logP / len^alpha in fp32, len = the tokens up to and
    including the first [SEP] (max_len without one), descending, ties to the lower beam index."""
    alpha = 0.0 if constraints is None else constraints.length_penalty
    if alpha == 0.0:
        return torch.sort(seq_logprob, 1, descending=True)[1]
    ended = outputs == EOS
    first = torch.where(ended.any(-1), ended.long().argmax(-1) + 1, max_len)                 # [b, beam]
    score = seq_logprob[..., 0] / torch.pow(first.to(torch.float32), torch.tensor(alpha, dtype=torch.float32, device=first.device))
    return torch.sort(score, dim=1, descending=True, stable=True)[1].unsqueeze(-1)


def _all_ended(source, t, max_len, unfinished):
    """asked every source.poll steps (a host synchronisation), never after the last step: has every row produced its [SEP]?"""
    return (t + 1) % source.poll == 0 and t + 1 < max_len and not bool(unfinished.any())


def decode_greedy(source, b, max_len, constraints=None, candidates=None):
    """VALOR.decode_greedy, model/pretrain.py:988-1028, mode 'greedy' (its logprobs are zeros in that mode) over a step source: the
    tokens stay on the device (the next step's input is this step's argmax); a finished row keeps producing [SEP] (:1005-1010), so
    the result does not depend on the step at which the loop leaves.
    constraints: one valor_logits_constrain launch on the step's logits, outside the captured step (history: sents, active: unfinished)."""
    dev = source.m.device
    sents = torch.full((b, max_len), EOS, dtype=torch.long, device=dev)
    logprobs = torch.zeros((b, max_len), device=dev)
    unfinished = torch.ones(b, dtype=torch.bool, device=dev)
    tok = None
    con = _constrainer(constraints, dev, candidates)
    for t in range(max_len):
        logits = source.step(tok)
        if con is not None:
            con(logits, sents, t, unfinished)
        wt = logits.max(1)[1]
        unfinished = unfinished & (wt != EOS)
        tok = torch.where(unfinished, wt, EOS)
        sents[:, t] = tok
        if _all_ended(source, t, max_len, unfinished):
            break
    return sents, logprobs


def decode_beam(source, b, beam, max_len, constraints=None, candidates=None):
    """VALOR.decode_beam / select / _adjust_tensor, model/pretrain.py:1054-1180, over a step source (rows beam-major): the selection
    arithmetic on the device, the chosen beams as the next step's `parent` rows. Step 0 reads the first b rows (a session runs `beam`
    identical copies of every sequence). A beam that produced [SEP] keeps its score for every candidate word (:1091-1094), so its V
    candidates tie and the reference's sort picks among them arbitrarily: sequences are only defined up to that choice once a beam has
    ended (the tokens behind [SEP] are dropped by decode_sequence :146-164 anyway).
    constraints: one valor_logits_constrain launch per step on the open beams' rows (the history follows the beams: `outputs`), and
    length_penalty at the final pick; in-search ranking stays the reference's. candidates: an AnswerSet -- the open rows are masked to
    the set's continuations (one valor_trie_constrain launch per step); the log-sum-exp of a row is the cross-entropy kernel's on the
    row BEFORE the mask, so a hypothesis keeps the model's sequence log-probability (score_candidates' law) and the candidates are
    ranked by it."""
    dev = source.m.device
    seq_logprob = torch.zeros((b, 1, 1), device=dev)
    seq_mask = torch.ones((b, beam, 1), device=dev)
    base = torch.arange(b, device=dev)
    outputs = torch.zeros((b, beam, max_len), dtype=torch.int64, device=dev)
    selected_words, tok, parent = None, None, None
    fused = beam_select_enabled() and beam <= 8
    con = _constrainer(constraints, dev, candidates)
    open_rows = torch.empty((beam, b), dtype=torch.bool, device=dev) if con is not None else None
    for t in range(max_len):
        cur = 1 if t == 0 else beam
        logits = source.step(tok, parent)
        V = logits.shape[-1]
        if t > 0:
            mask = (selected_words.view(b, cur) != EOS).float().unsqueeze(-1)
            seq_mask = seq_mask * mask
        lse_pre = row_lse(logits[:b * cur])[0] if candidates is not None else None
        if con is not None:                                          # the words so far sit in `outputs` as (sample, beam); the rows are beam-major
            if t > 0:
                torch.ne(seq_mask.view(b, beam).t(), 0, out=open_rows)
            con(logits[:b * cur], outputs, t, open_rows.view(-1) if t > 0 else None, b, beam * max_len, max_len)
        if fused:
            # (lse='kernel' -- the log-sum-exp inside the launch -- measured equal: 64 workgroups make three more passes over their rows)
            sel_logprob, sel_idx = beam_select(logits[:b * cur], b, cur, beam, seq_logprob, seq_mask, beam_major=True, lse="xent",
                                               lse_rows=lse_pre)
        else:
            word_logprob = (log_softmax_rows(logits[:b * cur]) if lse_pre is None else logits[:b * cur] - lse_pre[:, None])
            word_logprob = word_logprob.view(cur, b, -1).transpose(0, 1)
            cand = seq_logprob + word_logprob
            if t > 0:
                cand = seq_mask * cand + seq_logprob.expand_as(cand) * (1 - seq_mask)
            sel_logprob, sel_idx = torch.topk(cand.reshape(b, -1), beam, dim=-1, largest=True, sorted=True)   # select :1156-1159
        sel_beam = sel_idx // V
        selected_words = sel_idx - sel_beam * V
        seq_logprob = sel_logprob.unsqueeze(-1)
        seq_mask = torch.gather(seq_mask, 1, sel_beam.unsqueeze(-1))
        if t > 0:                                                    # the words so far follow their beams (:1101; one gather, not one per step)
            outputs = torch.gather(outputs, 1, sel_beam.unsqueeze(-1).expand(b, beam, max_len))
        outputs[:, :, t] = selected_words
        parent = (sel_beam.t() * b + base[None]).reshape(-1)        # row (k, s) continues row (sel_beam[s, k], s)
        tok = selected_words.t().reshape(-1)
    sort_idx = _final_beam_order(seq_logprob, outputs, max_len, constraints)
    outputs = torch.gather(outputs, 1, sort_idx.expand(b, beam, max_len))
    return outputs.contiguous()[:, 0]


# ------------------------------------------------------------------------------------------------ beam search with a finished-hypothesis pool
POOL_MAX_BEAM = 8                        # valor_beam_pool_step keeps 2 * beam candidates per thread in registers
_NO_INS = 2 ** 31 - 1                    # the insertion number of an empty pool entry


def inv_length_table(max_len, alpha):
    """inv[l] = 1 / l^alpha for l = 0 .. max_len (inv[0] = 1), computed in fp64 and rounded to fp32 once: the rank score of a hypothesis
    is the fp32 PRODUCT logP * inv[length], the same bits on the host and in the kernel (no powf, no division on the device)."""
    def one(l):
        try:
            return 1.0 / float(l) ** alpha
        except OverflowError:
            return 0.0
        except ZeroDivisionError:
            return float("inf")
    return torch.tensor([1.0] + [one(l) for l in range(1, max_len + 1)], dtype=torch.float64).to(torch.float32)


def _check_pool(who, b, beam, max_len, n_best=1, V=None, cur=None, t=None, eos=None):
    if int(beam) != beam or not 1 <= beam <= POOL_MAX_BEAM:
        raise ValueError(f"{who}: beam {beam!r} outside 1 .. {POOL_MAX_BEAM} (valor_beam_pool_step)")
    if int(n_best) != n_best or not 1 <= n_best <= beam:
        raise ValueError(f"{who}: n_best {n_best!r} outside 1 .. beam = {beam} (the pool holds `beam` finished hypotheses)")
    if int(max_len) != max_len or not 1 <= max_len <= 512:
        raise ValueError(f"{who}: max_len {max_len!r} outside 1 .. 512")
    if b < 0:
        raise ValueError(f"{who}: b = {b!r}")
    if V is not None:
        if not 1 <= cur <= beam:
            raise ValueError(f"{who}: cur {cur!r} outside 1 .. beam = {beam}")
        if cur * V < 2 * beam:
            raise ValueError(f"{who}: {cur} rows of {V} words hold fewer than 2 * beam = {2 * beam} candidates")
        if cur * V >= 2 ** 31 - 1:
            raise ValueError(f"{who}: {cur} x {V} candidates do not fit a 32-bit index")
        if not 0 <= t < max_len:
            raise ValueError(f"{who}: step {t!r} outside [0, max_len = {max_len})")
        if not 0 <= eos < V:
            raise ValueError(f"{who}: [SEP] = {eos!r} is no column of {V}")


class PoolState:
    """The arrays of one pool search (valor_beam_pool_step, include/valor_hip.h), on one device. Per sample: `beam` slots -- scores [b, beam]
    (-inf: a dead slot) and hist int64 [b, beam, max_len], each a ping-pong pair: step t reads [t % 2] and writes [(t + 1) % 2] -- the
    pool of at most `beam` finished hypotheses (pool_seq, pool_logprob, pool_rank, pool_len, pool_ins, pool_cnt = (entries, insertions)),
    `done` [b], `floor` (a logit at or below it is no continuation: -inf, or TRIE_FLOOR inside an answer set), and what a step leaves for the next one: tok / parent int64 [beam * b] beam-major, active uint8 [beam, b]."""
    FIELDS = ("scores", "hist", "inv", "pool_seq", "pool_logprob", "pool_rank", "pool_len", "pool_ins", "pool_cnt", "done", "tok", "parent",
              "active")

    def __init__(self, b, beam, max_len, alpha=0.0, device="cpu", eos=None, floor=-float("inf")):
        _check_pool("PoolState", b, beam, max_len)
        self.floor = float(floor)                      # TRIE_FLOOR inside an answer set: a floored column is no continuation
        self.b, self.beam, self.max_len, self.alpha = int(b), int(beam), int(max_len), float(alpha)
        self.eos = EOS if eos is None else int(eos)
        ninf = -float("inf")
        mk = lambda shape, fill, dt: torch.full(shape, fill, dtype=dt, device=device)
        self.scores = [mk((b, beam), ninf, torch.float32) for _ in range(2)]
        self.scores[0][:, 0] = 0.0
        self.hist = [mk((b, beam, max_len), 0, torch.int64) for _ in range(2)]
        self.inv = inv_length_table(max_len, self.alpha).to(device)
        self.pool_seq = mk((b, beam, max_len), self.eos, torch.int64)
        self.pool_logprob, self.pool_rank = mk((b, beam), ninf, torch.float32), mk((b, beam), ninf, torch.float32)
        self.pool_len, self.pool_ins = mk((b, beam), 0, torch.int32), mk((b, beam), _NO_INS, torch.int32)
        self.pool_cnt = mk((b, 2), 0, torch.int32)
        self.done = mk((b,), 0, torch.uint8)
        self.tok, self.parent = mk((beam * b,), self.eos, torch.int64), torch.arange(beam * b, dtype=torch.int64, device=device)
        self.active = mk((beam, b), 0, torch.uint8)

    def to(self, device):
        """a copy on `device`"""
        import copy
        out = copy.copy(self)
        for k in self.FIELDS:
            v = getattr(self, k)
            setattr(out, k, [x.to(device, copy=True) for x in v] if isinstance(v, list) else v.to(device, copy=True))
        return out

    def arrays(self):
        """{name: host tensor} of every array (the pairs as name0 / name1): what a comparison walks"""
        out = {}
        for k in self.FIELDS:
            v = getattr(self, k)
            for i, x in enumerate(v if isinstance(v, list) else [v]):
                out[k + (str(i) if isinstance(v, list) else "")] = x.detach().cpu()
        return out

    def result(self, n_best):
        """the pool sorted by rank score descending, equal scores by earlier insertion -> (seqs int64 [b, n, L], rank fp32 [b, n],
        logprob fp32 [b, n], length int64 [b, n]); a missing entry is an all-[SEP] row with rank and logprob -inf and length 0"""
        n, L = int(n_best), self.max_len
        by_age = torch.sort(self.pool_ins, dim=1, stable=True)[1]
        order = torch.gather(by_age, 1, torch.sort(torch.gather(self.pool_rank, 1, by_age), dim=1, descending=True, stable=True)[1])[:, :n]
        seqs = torch.gather(self.pool_seq, 1, order[:, :, None].expand(self.b, n, L))
        return (seqs.contiguous(), torch.gather(self.pool_rank, 1, order), torch.gather(self.pool_logprob, 1, order),
                torch.gather(self.pool_len, 1, order).to(torch.int64))


def beam_pool_step(logits, lse, state, t, cur, early_stopping=False, beam_major=True):
    """one step of the pool search in ONE launch (valor_beam_pool_step; the law: include/valor_hip.h, restated by beam_pool_step_host):
    logits fp32 [b * cur, V] (unit column stride; rows beam-major r = k * b + s, or sample-major r = s * cur + k), lse fp32 [b * cur]
    (the rows' log-sum-exp as the caller has it: row_lse), state: a PoolState on the logits' device, updated in place (scores / hist
    [(t + 1) % 2], tok, parent, active, the pool, done). Anything the kernel cannot do raises ValueError: there is no torch path."""
    st = state
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.stride(1) != 1 or lse.dtype != torch.float32 or not lse.is_contiguous():
        raise ValueError("beam_pool_step: logits fp32 [rows, V] with unit column stride and lse fp32 [rows]")
    V = logits.shape[1]
    _check_pool("beam_pool_step", st.b, st.beam, st.max_len, 1, V, cur, t, st.eos)
    if logits.shape[0] != st.b * cur or lse.numel() != st.b * cur:
        raise ValueError(f"beam_pool_step: {logits.shape[0]} rows / {lse.numel()} lse values for b * cur = {st.b * cur}")
    K._check_gpu(logits, lse, st.done)
    i, o = t % 2, (t + 1) % 2
    rs_s, rs_k = (1, st.b) if beam_major else (cur, 1)
    lib.call("valor_beam_pool_step", _st(), logits.data_ptr(), logits.stride(0), rs_s, rs_k, lse.data_ptr(), st.scores[i].data_ptr(),
             st.hist[i].data_ptr(), st.inv.data_ptr(), st.b, cur, V, st.beam, st.max_len, t, st.eos, st.floor, int(st.alpha > 0.0), int(bool(early_stopping)),
             st.scores[o].data_ptr(), st.hist[o].data_ptr(), st.tok.data_ptr(), st.parent.data_ptr(), st.active.data_ptr(),
             st.pool_seq.data_ptr(), st.pool_logprob.data_ptr(), st.pool_rank.data_ptr(), st.pool_len.data_ptr(), st.pool_ins.data_ptr(),
             st.pool_cnt.data_ptr(), st.done.data_ptr())
    return st


def beam_pool_step_host(logits, lse, state, t, cur, early_stopping=False, beam_major=True):
    """THE LAW of one step of the pool search (include/valor_hip.h, valor_beam_pool_step), on the host in fp32: beam_pool_step's
    arguments with a PoolState of host tensors, updated in place; logits / lse may live anywhere and are not modified. Every value
    is one rounded fp32 operation in the kernel's order -- c = c_k + (z - lse), rank = c * inv[length], the bound c_0 * inv[..] --
    so the kernel agrees with it bit for bit. The early-exit bound (rule 6) is the usual one taken literally: the best an open
    hypothesis can still reach is its own score at the most favourable length, which is exact only while every further
    log-probability is <= 0 (true of log-softmax rows; inside an answer set the scores are those of the unmasked rows, also <= 0)."""
    st = state
    z = logits.detach().to(device="cpu", dtype=torch.float32)
    l = lse.detach().to(device="cpu", dtype=torch.float32).reshape(-1)
    b, K_, L, eos = st.b, st.beam, st.max_len, st.eos
    V = z.shape[1]
    _check_pool("beam_pool_step_host", b, K_, L, 1, V, cur, t, eos)
    if z.shape[0] != b * cur or l.numel() != b * cur:
        raise ValueError(f"beam_pool_step_host: {z.shape[0]} rows / {l.numel()} lse values for b * cur = {b * cur}")
    i, o = t % 2, (t + 1) % 2
    sc_in, sc_out, h_in, h_out = st.scores[i], st.scores[o], st.hist[i], st.hist[o]
    ninf = -float("inf")
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)
    for s in range(b):
        if bool(st.done[s]):                                         # rule 7: frozen
            sc_out[s], h_out[s] = sc_in[s], h_in[s]
            for k in range(K_):
                st.tok[k * b + s], st.parent[k * b + s], st.active[k, s] = eos, k * b + s, 0
            continue
        cand = torch.full((cur, V), ninf, dtype=torch.float32)
        for k in range(cur):
            if float(sc_in[s, k]) > ninf:                            # rule 1 (a dead slot supplies nothing)
                r = k * b + s if beam_major else s * cur + k
                cand[k] = torch.where(z[r] > st.floor, sc_in[s, k] + (z[r] - l[r]), f32(ninf))
        flat = cand.reshape(-1)
        flat = torch.where(flat.isnan(), f32(ninf), flat)
        val, idx = torch.sort(flat, descending=True, stable=True)    # rule 2: value descending, equal values in index order
        taken = [(val[j].clone(), int(idx[j])) for j in range(min(2 * K_, flat.numel())) if float(val[j]) > ninf]
        pn, pnext = int(st.pool_cnt[s, 0]), int(st.pool_cnt[s, 1])
        slots = []                                                   # (score, parent slot, token)
        for rho, (c, ix) in enumerate(taken):                        # rule 3
            if len(slots) == K_:
                break
            k, w = divmod(ix, V)
            ends = w == eos
            if ends and rho >= K_:
                continue
            if not ends:
                slots.append((c, k, w))
                if t < L - 1:
                    continue
            length = t + 1 if ends else L
            rank = c * st.inv[length]
            dst = -1
            if pn < K_:                                              # rule 4
                dst, pn = pn, pn + 1
            else:
                worst = 0
                for j in range(1, K_):
                    rj, rw = float(st.pool_rank[s, j]), float(st.pool_rank[s, worst])
                    if rj < rw or (rj == rw and int(st.pool_ins[s, j]) > int(st.pool_ins[s, worst])):
                        worst = j
                if float(rank) > float(st.pool_rank[s, worst]):
                    dst = worst
            if dst >= 0:
                st.pool_logprob[s, dst], st.pool_rank[s, dst], st.pool_len[s, dst], st.pool_ins[s, dst] = c, rank, length, pnext
                pnext += 1
                st.pool_seq[s, dst, :t] = h_in[s, k, :t]
                st.pool_seq[s, dst, t] = w
                st.pool_seq[s, dst, t + 1:] = eos
        filled = len(slots)
        slots += [(f32(ninf), j, eos) for j in range(filled, K_)]    # rule 5
        d = True
        if t < L - 1:                                                # rule 6
            d = filled == 0
            if not d and pn == K_:
                d = bool(early_stopping) or float(st.pool_rank[s].min()) >= float(slots[0][0] * st.inv[L if st.alpha > 0.0 else t + 2])
        st.pool_cnt[s, 0], st.pool_cnt[s, 1], st.done[s] = pn, pnext, int(d)
        for j, (c, k, w) in enumerate(slots):
            sc_out[s, j] = c
            row = h_in[s, k].clone()
            row[t] = w
            h_out[s, j] = row
            st.tok[j * b + s], st.parent[j * b + s] = w, k * b + s
            st.active[j, s] = int(not d and float(c) > ninf)
    return st


# ------------------------------------------------------------------------------------------------ diverse beam search: beam groups
def diversity_table(beam, diversity_penalty):
    """pen[n] = diversity_penalty * n for n = 0 .. beam, the product in fp64 rounded to fp32 once (pen[0] = 0): the selection key of a
    word that n earlier slots of the step took is the fp32 DIFFERENCE c - pen[n], the same bits on the host and in the kernel (no
    multiply on the device, as inv_length_table)."""
    lam = float(diversity_penalty)
    return torch.tensor([0.0] + [lam * n for n in range(1, int(beam) + 1)], dtype=torch.float64).to(torch.float32)


def _check_groups(who, beam, groups, diversity_penalty=0.0, V=None, cur=None):
    if int(groups) != groups or not 1 <= groups <= beam or beam % groups:
        raise ValueError(f"{who}: num_beam_groups {groups!r} must divide the beam {beam}")
    lam = float(diversity_penalty)
    if not (0.0 <= lam < float("inf")):
        raise ValueError(f"{who}: diversity_penalty {diversity_penalty!r} must be finite and >= 0")
    if V is not None:
        if cur not in (1, beam):
            raise ValueError(f"{who}: cur {cur!r} is neither 1 (the first step) nor the beam {beam}")
        if V < 2 * (beam // groups):
            raise ValueError(f"{who}: {V} words hold fewer than 2 * beam / groups = {2 * (beam // groups)} candidates")


class GroupPoolState(PoolState):
    """The arrays of one diverse (group) pool search (valor_beam_group_step, include/valor_hip.h): PoolState's, with the `beam` slots and
    the `beam` pool entries split into `groups` ranges of beam / groups (group g owns g * Kg .. (g + 1) * Kg - 1 of both), pool_cnt int32
    [b, groups, 2] = (entries held, insertions) per group, gdone uint8 [b, groups] (done[s] = all of gdone[s]) and pen fp32 [beam + 1],
    the diversity_table of the penalty."""
    FIELDS = PoolState.FIELDS + ("gdone", "pen")

    def __init__(self, b, beam, groups, max_len, alpha=0.0, device="cpu", eos=None, floor=-float("inf"), diversity_penalty=0.0):
        super().__init__(b, beam, max_len, alpha, device, eos, floor)
        _check_groups("GroupPoolState", beam, groups, diversity_penalty)
        self.groups, self.diversity_penalty = int(groups), float(diversity_penalty)
        self.pool_cnt = torch.zeros((b, self.groups, 2), dtype=torch.int32, device=device)
        self.gdone = torch.zeros((b, self.groups), dtype=torch.uint8, device=device)
        self.pen = diversity_table(beam, diversity_penalty).to(device)

    def result(self, n_best):
        """every group's pool sorted as PoolState.result sorts one (rank score descending, equal scores by earlier insertion), then the
        entries by their PLACE within their group (0 = the group's best), within one place by rank score descending, equal scores by
        group index: entry 0 is the overall best and the first `groups` entries are one hypothesis per group
        -> (seqs int64 [b, n, L], rank fp32 [b, n], logprob fp32 [b, n], length int64 [b, n], group int64 [b, n])"""
        n, L, G = int(n_best), self.max_len, self.groups
        Kg = self.beam // G
        ins, rank = self.pool_ins.view(self.b, G, Kg), self.pool_rank.view(self.b, G, Kg)
        by_age = torch.sort(ins, dim=2, stable=True)[1]
        place = torch.gather(by_age, 2, torch.sort(torch.gather(rank, 2, by_age), dim=2, descending=True, stable=True)[1])   # [b, G, place]
        place = place + torch.arange(G, device=place.device).view(1, G, 1) * Kg                                               # pool entries
        rank_at = torch.gather(self.pool_rank, 1, place.reshape(self.b, -1)).view(self.b, G, Kg)
        by_group = torch.sort(rank_at, dim=1, descending=True, stable=True)[1]                                                # [b, ., place]
        order = torch.gather(place, 1, by_group).transpose(1, 2).reshape(self.b, -1)[:, :n]
        seqs = torch.gather(self.pool_seq, 1, order[:, :, None].expand(self.b, n, L))
        return (seqs.contiguous(), torch.gather(self.pool_rank, 1, order), torch.gather(self.pool_logprob, 1, order),
                torch.gather(self.pool_len, 1, order).to(torch.int64), order // Kg)


def beam_group_step(logits, lse, state, t, cur, early_stopping=False, beam_major=True):
    """one step of the group pool search in ONE launch (valor_beam_group_step; the law: include/valor_hip.h, restated by
    beam_group_step_host): beam_pool_step's arguments with a GroupPoolState on the logits' device, updated in place (gdone besides).
    cur is 1 (the first step: every group reads the one row of slot 0) or the beam. Anything the kernel cannot do raises ValueError:
    there is no torch path."""
    st = state
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.stride(1) != 1 or lse.dtype != torch.float32 or not lse.is_contiguous():
        raise ValueError("beam_group_step: logits fp32 [rows, V] with unit column stride and lse fp32 [rows]")
    V = logits.shape[1]
    _check_pool("beam_group_step", st.b, st.beam, st.max_len, 1, V, cur, t, st.eos)
    _check_groups("beam_group_step", st.beam, st.groups, st.diversity_penalty, V, cur)
    if logits.shape[0] != st.b * cur or lse.numel() != st.b * cur:
        raise ValueError(f"beam_group_step: {logits.shape[0]} rows / {lse.numel()} lse values for b * cur = {st.b * cur}")
    K._check_gpu(logits, lse, st.done)
    i, o = t % 2, (t + 1) % 2
    rs_s, rs_k = (1, st.b) if beam_major else (cur, 1)
    lib.call("valor_beam_group_step", _st(), logits.data_ptr(), logits.stride(0), rs_s, rs_k, lse.data_ptr(), st.scores[i].data_ptr(),
             st.hist[i].data_ptr(), st.inv.data_ptr(), st.pen.data_ptr(), st.b, cur, V, st.beam, st.groups, st.max_len, t, st.eos, st.floor,
             int(st.alpha > 0.0), int(bool(early_stopping)), st.scores[o].data_ptr(), st.hist[o].data_ptr(), st.tok.data_ptr(),
             st.parent.data_ptr(), st.active.data_ptr(), st.pool_seq.data_ptr(), st.pool_logprob.data_ptr(), st.pool_rank.data_ptr(),
             st.pool_len.data_ptr(), st.pool_ins.data_ptr(), st.pool_cnt.data_ptr(), st.gdone.data_ptr(), st.done.data_ptr())
    return st


def beam_group_step_host(logits, lse, state, t, cur, early_stopping=False, beam_major=True):
    """THE LAW of one step of the group pool search (include/valor_hip.h, valor_beam_group_step), on the host in fp32: beam_group_step's
    arguments with a GroupPoolState of host tensors, updated in place. The groups of a sample are searched one after another; a group
    is beam_pool_step_host's law on its own slots and pool range, except that the candidates are ORDERED by the key
    a = c - pen[n_w] (n_w: the new open slots that earlier groups filled with word w at this step) while a slot, an offer and the
    bound carry the unpenalised c. Every value is one rounded fp32 operation in the kernel's order, so the kernel agrees bit for bit."""
    st = state
    z = logits.detach().to(device="cpu", dtype=torch.float32)
    l = lse.detach().to(device="cpu", dtype=torch.float32).reshape(-1)
    b, K_, G, L, eos = st.b, st.beam, st.groups, st.max_len, st.eos
    Kg = K_ // G
    V = z.shape[1]
    _check_pool("beam_group_step_host", b, K_, L, 1, V, cur, t, eos)
    _check_groups("beam_group_step_host", K_, G, st.diversity_penalty, V, cur)
    if z.shape[0] != b * cur or l.numel() != b * cur:
        raise ValueError(f"beam_group_step_host: {z.shape[0]} rows / {l.numel()} lse values for b * cur = {b * cur}")
    i, o = t % 2, (t + 1) % 2
    sc_in, sc_out, h_in, h_out = st.scores[i], st.scores[o], st.hist[i], st.hist[o]
    ninf = -float("inf")
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)

    def freeze(s, k):
        sc_out[s, k], h_out[s, k] = sc_in[s, k], h_in[s, k]
        st.tok[k * b + s], st.parent[k * b + s], st.active[k, s] = eos, k * b + s, 0

    for s in range(b):
        if bool(st.done[s]):                                         # a done sample is frozen
            for k in range(K_):
                freeze(s, k)
            continue
        count = torch.zeros(V, dtype=torch.int64)                    # n_w: the words the earlier groups' new open slots took
        for g in range(G):
            lo = g * Kg
            if bool(st.gdone[s, g]):                                 # a done group is frozen and lends no words
                for k in range(lo, lo + Kg):
                    freeze(s, k)
                continue
            ks = [0] if cur == 1 else list(range(lo, lo + Kg))       # the first step: every group reads the one row of slot 0
            cand = torch.full((len(ks), V), ninf, dtype=torch.float32)
            for j, k in enumerate(ks):
                if float(sc_in[s, k]) > ninf:
                    r = k * b + s if beam_major else s * cur + k
                    cand[j] = torch.where(z[r] > st.floor, sc_in[s, k] + (z[r] - l[r]), f32(ninf))
            key = (cand - st.pen[count][None, :]).reshape(-1)        # one fp32 subtraction; pen[0] = 0 leaves c as it is
            key = torch.where(key.isnan(), f32(ninf), key)
            val, idx = torch.sort(key, descending=True, stable=True)
            taken = [(cand.reshape(-1)[int(idx[j])].clone(), ks[int(idx[j]) // V], int(idx[j]) % V)
                     for j in range(min(2 * Kg, key.numel())) if float(val[j]) > ninf]
            pn, pnext = int(st.pool_cnt[s, g, 0]), int(st.pool_cnt[s, g, 1])
            slots = []                                               # (score, parent slot, token)
            for rho, (c, k, w) in enumerate(taken):
                if len(slots) == Kg:
                    break
                ends = w == eos
                if ends and rho >= Kg:
                    continue
                if not ends:
                    slots.append((c, k, w))
                    if t < L - 1:
                        continue
                length = t + 1 if ends else L
                rank = c * st.inv[length]
                dst = -1
                if pn < Kg:
                    dst, pn = pn, pn + 1
                else:
                    worst = 0
                    for j in range(1, Kg):
                        rj, rw = float(st.pool_rank[s, lo + j]), float(st.pool_rank[s, lo + worst])
                        if rj < rw or (rj == rw and int(st.pool_ins[s, lo + j]) > int(st.pool_ins[s, lo + worst])):
                            worst = j
                    if float(rank) > float(st.pool_rank[s, lo + worst]):
                        dst = worst
                if dst >= 0:
                    e = lo + dst
                    st.pool_logprob[s, e], st.pool_rank[s, e], st.pool_len[s, e], st.pool_ins[s, e] = c, rank, length, pnext
                    pnext += 1
                    st.pool_seq[s, e, :t] = h_in[s, k, :t]
                    st.pool_seq[s, e, t] = w
                    st.pool_seq[s, e, t + 1:] = eos
            filled = len(slots)
            for c, _, w in slots:
                count[w] += 1
            d = True
            if t < L - 1:
                d = filled == 0
                if not d and pn == Kg:                               # the bound: the group's largest new score (need not be its slot 0)
                    top = max(float(c) for c, _, _ in slots)
                    d = bool(early_stopping) or float(st.pool_rank[s, lo:lo + Kg].min()) >= float(f32(top) * st.inv[L if st.alpha > 0.0 else t + 2])
            slots += [(f32(ninf), lo + j, eos) for j in range(filled, Kg)]
            st.pool_cnt[s, g, 0], st.pool_cnt[s, g, 1], st.gdone[s, g] = pn, pnext, int(d)
            for j, (c, k, w) in enumerate(slots):
                sc_out[s, lo + j] = c
                row = h_in[s, k].clone()
                row[t] = w
                h_out[s, lo + j] = row
                st.tok[(lo + j) * b + s], st.parent[(lo + j) * b + s] = w, k * b + s
                st.active[lo + j, s] = int(not d and float(c) > ninf)
        st.done[s] = int(bool(st.gdone[s].all()))
    return st


def _pool_lse(z):
    return torch.logsumexp(z.to(torch.float32), 1)


def decode_beam_pool_host(script_or_source, b, beam, max_len, constraints=None, candidates=None, n_best=1, early_stopping=False, lse=None,
                          eos=None, num_beam_groups=1, diversity_penalty=0.0):
    """THE LAW of the pool search as a whole: decode_beam_pool's loop on the host, built on beam_pool_step_host, with constrain_rows_host /
    trie_rows_host in the place of the launches. script_or_source: a list of max_len logits tensors [>= b * beam, V] (step t reads the
    first b * cur rows, beam-major: a scripted decoder) or a step source (source.step(tok, parent)). lse: rows -> their log-sum-exp
    (None: torch.logsumexp in fp32; pass the cross-entropy kernel's, row_lse, to reproduce a device run bit for bit). It asks after every
    step whether all samples are done; a done sample is frozen, so the result does not depend on when a loop leaves.
    num_beam_groups > 1: the same loop on a GroupPoolState with beam_group_step_host in the place of beam_pool_step_host.
    -> PoolState.result(n_best): (seqs, rank, logprob, length); with groups GroupPoolState.result(n_best): the group index besides."""
    eos = EOS if eos is None else eos
    _check_pool("decode_beam_pool_host", b, beam, max_len, n_best)
    grouped = _grouped("decode_beam_pool_host", beam, num_beam_groups, diversity_penalty)
    alpha = 0.0 if constraints is None else constraints.length_penalty
    floor = -float("inf") if candidates is None else TRIE_FLOOR
    st = (GroupPoolState(b, beam, num_beam_groups, max_len, alpha, "cpu", eos, floor, diversity_penalty) if grouped else
          PoolState(b, beam, max_len, alpha, "cpu", eos, floor))
    if candidates is not None:
        _no_logits_rules(constraints)
    rules = constraints is not None and not constraints.logits_off
    lse = _pool_lse if lse is None else lse
    scripted = isinstance(script_or_source, (list, tuple))
    tok = parent = None
    for t in range(max_len):
        cur = 1 if t == 0 else beam
        if scripted:
            z = script_or_source[t][:b * cur]
        else:
            dev = script_or_source.m.device
            z = script_or_source.step(None if tok is None else tok.to(dev), None if parent is None else parent.to(dev))[:b * cur]
        hist = st.hist[t % 2].transpose(0, 1).reshape(beam * b, max_len)              # row k * b + s: the words of slot k of sample s
        active = None if t == 0 else st.active.reshape(-1)
        l = None
        if candidates is not None:                                                    # the log-sum-exp of the row BEFORE its mask
            l = lse(z).detach().cpu()
            z = trie_rows_host(z, hist, t, candidates, eos, b, active)
        elif rules:
            z = constrain_rows_host(z, hist, t, constraints, eos, active)
        if l is None:
            l = lse(z).detach().cpu()
        (beam_group_step_host if grouped else beam_pool_step_host)(z, l, st, t, cur, early_stopping)
        tok, parent = st.tok.clone(), st.parent.clone()
        if t + 1 < max_len and bool(st.done.all()):
            break
    return st.result(n_best)


def _grouped(who, beam, num_beam_groups, diversity_penalty):
    """whether a pool search runs in beam groups (num_beam_groups > 1), after the checks of the two arguments"""
    _check_groups(who, beam, num_beam_groups, diversity_penalty)
    if num_beam_groups == 1 and float(diversity_penalty) > 0.0:
        raise ValueError(f"{who}: diversity_penalty {diversity_penalty!r} needs num_beam_groups > 1 (one group has nobody to differ from)")
    return num_beam_groups > 1


def decode_beam_pool(source, b, beam, max_len, constraints=None, candidates=None, n_best=1, early_stopping=False, num_beam_groups=1,
                     diversity_penalty=0.0):
    """Beam search with a pool of finished hypotheses over a step source (rows beam-major), the search captioning users expect: a
    hypothesis that produced [SEP] leaves the beam for a pool of at most `beam` finished ones, the beam stays `beam` OPEN hypotheses
    wide, the pool is ranked by logP * inv[length] (inv[l] = 1 / l^length_penalty: the ranking acts while the search runs), and a
    sample is done as soon as no open hypothesis can still enter its pool (early_stopping: as soon as the pool is full). The law:
    beam_pool_step_host / decode_beam_pool_host, bit for bit.
    Per step: the source's step, the constrainer's launch when a rule is on (valor_logits_constrain / valor_trie_constrain, as in
    decode_beam; with an AnswerSet the log-sum-exp is that of the row BEFORE its mask), the cross-entropy kernel's row log-sum-exp, and
    ONE valor_beam_pool_step launch that does the selection, the pool update, the history reorder and the next step's tok / parent /
    active rows. Nothing is read back except `done`, every source.poll steps and never after the last one (_all_ended's pattern); the
    loop leaves when every sample is done.
    -> (seqs int64 [b, n_best, max_len] padded with [SEP], rank fp32 [b, n_best], logprob fp32 [b, n_best], length int64 [b, n_best]),
    best first; fewer than n_best hypotheses (possible only inside an answer set) leave all-[SEP] rows with scores -inf and length 0.
    beam outside 1 .. 8, n_best outside 1 .. beam, a vocabulary below 2 * beam raise ValueError: there is no torch path.
    num_beam_groups = G > 1 (G divides beam), diversity_penalty >= 0: diverse beam search (Vijayakumar et al.). The beam is G groups of
    beam / G slots, each with its own pool range, searched one after another inside the step's ONE valor_beam_group_step launch; a
    later group orders its candidates by c - diversity_penalty * (the number of new open slots of earlier groups that took the word at
    this step). The penalty steers the selection only: scores, ranks and the returned log-probabilities stay true log-probabilities
    (HF-style implementations fold the penalty into the running score). The law: beam_group_step_host. The result gains a fifth
    entry, the group of every hypothesis, and is ordered as GroupPoolState.result orders it (the first G: one per group)."""
    dev = source.m.device
    _check_pool("decode_beam_pool", b, beam, max_len, n_best)
    grouped = _grouped("decode_beam_pool", beam, num_beam_groups, diversity_penalty)
    alpha, floor = 0.0 if constraints is None else constraints.length_penalty, -float("inf") if candidates is None else TRIE_FLOOR
    st = (GroupPoolState(b, beam, num_beam_groups, max_len, alpha, dev, floor=floor, diversity_penalty=diversity_penalty) if grouped else
          PoolState(b, beam, max_len, alpha, dev, floor=floor))
    step = beam_group_step if grouped else beam_pool_step
    con = _constrainer(constraints, dev, candidates)
    tok = parent = None
    for t in range(max_len):
        cur = 1 if t == 0 else beam
        logits = source.step(tok, parent)[:b * cur]
        lse = row_lse(logits)[0] if candidates is not None else None
        if con is not None:                                          # the words so far sit in `hist` as (sample, slot); the rows are beam-major
            con(logits, st.hist[t % 2], t, st.active.view(-1) if t > 0 else None, b, beam * max_len, max_len)
        if lse is None:
            lse = row_lse(logits)[0]
        step(logits, lse, st, t, cur, early_stopping)
        tok, parent = st.tok, st.parent
        if (t + 1) % source.poll == 0 and t + 1 < max_len and bool(st.done.all()):
            break
    return st.result(n_best)


@contextlib.contextmanager
def no_gc():
    """Keep Python's cyclic collector out of a decoding step's capture. A dead cycle that still holds device resources -- an earlier model
    with its decoding sessions: their hipGraphs, private pools, events -- is freed whenever the collector happens to run; inside a capture
    (error mode "global") those frees are illegal calls that end the process from a destructor, and torch.cuda.graph no longer collects
    before it begins a capture. The collector is switched off for the capture's duration; the cycle goes afterwards."""
    on = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if on:
            gc.enable()


class SampleStream:
    """the Philox stream of the sampled decode: plain ints (like DeviceTokenMasker). Each decode call draws under its own key, derived
    from (seed, data-parallel rank, call index): ranks draw different samples and a rerun with the same seed draws the same ones. Inside
    a call the counter `offset` advances by R * ceil(V / 4) per step (every group and step reads a window of its own)."""

    def __init__(self, seed=42):
        self.seed = int(seed)
        self.calls = 0
        self.key = None
        self.offset = 0

    def _key_of(self, call):
        import numpy as np
        from .model.valor import _dp_rank
        w = np.random.SeedSequence(self.seed, spawn_key=(_dp_rank(), 2, call)).generate_state(2, np.uint32)
        return int(w[0]) | int(w[1]) << 32

    def begin_call(self):
        self.key = self._key_of(self.calls)
        self.offset = 0
        self.calls += 1
        return self

    def state(self):
        """the ints the next draw depends on (a checkpoint entry); the key is a function of (seed, rank, calls) and is not stored"""
        return {"seed": self.seed, "calls": self.calls, "offset": self.offset}

    def set_state(self, st):
        self.seed, self.calls, self.offset = int(st["seed"]), int(st["calls"]), int(st["offset"])
        self.key = self._key_of(self.calls - 1) if self.calls > 0 else None       # the key of the call that was under way

    def take(self, R, V):
        off = self.offset
        self.offset += R * ((V + 3) // 4)
        return self.key, off


def sampler_of(model):
    """the model's SampleStream (seeded from opts.seed at first use)"""
    s = model.__dict__.get("_sample_stream")
    if s is None:
        from .model.valor import _opt
        s = model.__dict__["_sample_stream"] = SampleStream(int(_opt(model.opts, "seed", 42)))
    return s


def sampler_state(model):
    """state() of the model's SampleStream, or None while nothing has sampled yet (the stream is created at first use)"""
    s = model.__dict__.get("_sample_stream")
    return None if s is None else s.state()


def set_sampler_state(model, st):
    """restore sampler_state(): None = a model that had not sampled yet (the stream is dropped and re-created from opts.seed at first use)"""
    if st is None:
        model.__dict__.pop("_sample_stream", None)
    else:
        sampler_of(model).set_state(st)


class Sampling:
    """the filters of the sampled decode: temperature (the logits are divided by it), top_k (0: off; ties at the k-th value are kept),
    top_p (the nucleus, over what top-k left; 1: off). The defaults are all off: the unmodified softmax."""
    __slots__ = ("temperature", "top_k", "top_p")

    def __init__(self, temperature=1.0, top_k=0, top_p=1.0):
        temperature, top_p = float(temperature), float(top_p)
        if temperature == 0.0:
            raise ValueError("Sampling: temperature 0 is the arg max -- use mode='greedy'")
        if not (temperature > 0.0 and temperature != float("inf")):
            raise ValueError(f"Sampling: temperature {temperature!r} must be a finite number > 0")
        if int(top_k) != top_k or top_k < 0:
            raise ValueError(f"Sampling: top_k {top_k!r} must be an integer >= 0 (0: off)")
        if not (0.0 < top_p <= 1.0):
            raise ValueError(f"Sampling: top_p {top_p!r} must be in (0, 1] (1: off)")
        self.temperature, self.top_k, self.top_p = temperature, int(top_k), top_p

    @property
    def off(self):
        return self.temperature == 1.0 and self.top_k == 0 and self.top_p == 1.0

    @property
    def inv_temperature(self):
        """1 / temperature rounded to fp32: what the kernel multiplies the logits by"""
        return float(torch.tensor(1.0 / self.temperature, dtype=torch.float32))

    def __repr__(self):
        return f"Sampling(temperature={self.temperature}, top_k={self.top_k}, top_p={self.top_p})"


def filter_row(y, top_k=0, top_p=1.0):
    """Rules 2 and 3 of valor_sample_tokens_filtered (include/valor_hip.h) restated on the host for ONE row y (any float dtype, already
    multiplied by 1 / temperature, no NaN) -> (kept, cut): the size of the kept set S and min over S of y (kept 0, cut NaN when no column
    is above -inf). The masses are summed in fp64."""
    y = y.detach().double().cpu().reshape(-1)
    vals = torch.sort(y[y > -float("inf")], descending=True).values
    if vals.numel() == 0:
        return 0, float("nan")
    if 1 <= top_k < vals.numel():
        vals = vals[vals >= vals[top_k - 1]]
    if top_p < 1.0:
        mass = torch.cumsum(torch.exp(vals - vals[0]), 0)
        first = int((mass >= top_p * mass[-1]).nonzero()[0])
        vals = vals[vals >= vals[first]]
    return int(vals.numel()), float(vals[-1])


def _draw_step(logits, stream, sampling, unfinished, tok, sents_t, logprobs_t):
    """one sampler launch: valor_sample_tokens, or the filtered kernel when a filter is on"""
    seed, off = stream.take(logits.shape[0], logits.shape[1])
    if sampling is None or sampling.off:
        K.sample_tokens(logits, seed, off, EOS, unfinished, tok, sents_t, logprobs_t)
    else:
        K.sample_tokens_filtered(logits, seed, off, EOS, unfinished, tok, sents_t, logprobs_t, sampling.inv_temperature, sampling.top_k,
                                 sampling.top_p)


def _skip_windows(stream, candidates, R, V, steps):
    """inside an answer set every row ends after a few tokens and the two step sources leave the sampled loop at different steps
    (`poll`): the call still consumes its max_len counter windows, so the next group draws the same numbers on either source. Without
    an answer set nothing is skipped: the stream stays what it was before answer sets existed."""
    if candidates is not None:
        for _ in range(steps):
            stream.take(R, V)


def decode_sample(source, b, max_len, stream, sampling=None, constraints=None, candidates=None):
    """VALOR.decode_greedy mode 'sample' (pretrain.py:1005-1020) over a step source: one step, then one valor_sample_tokens launch that
    draws from softmax(logits), writes the logP of the draw and does the [SEP] bookkeeping. The tokens stay on the device, as in
    decode_greedy. -> (sents int64 [b, max_len], logprobs fp32 [b, max_len]); after a row's first [SEP] its tokens are [SEP] and its
    logprobs 0. sampling: a Sampling (None or all off: the unmodified softmax); the sampler
    launch sits outside the captured step and takes its parameters by value, so a kept session serves any setting. constraints come
    first (valor_logits_constrain on the step's logits): temperature / top-k / top-p and the logP see what the constraints left."""
    dev = source.m.device
    sents = torch.full((b, max_len), EOS, dtype=torch.long, device=dev)
    logprobs = torch.zeros((b, max_len), device=dev)
    unfinished = torch.ones(b, dtype=torch.bool, device=dev)
    tok = torch.empty(b, dtype=torch.long, device=dev)
    con = _constrainer(constraints, dev, candidates)
    for t in range(max_len):
        logits = source.step(None if t == 0 else tok)
        if con is not None:
            con(logits, sents, t, unfinished)
        _draw_step(logits, stream, sampling, unfinished, tok, sents[:, t], logprobs[:, t])
        if _all_ended(source, t, max_len, unfinished):
            break
    _skip_windows(stream, candidates, b, logits.shape[1], max_len - t - 1)
    return sents, logprobs


def _decode_groups(model, groups, b, kv_layers, ranges, prompt, beam, max_len, stream=None, sampling=None, constraints=None, candidates=None,
                   pool=None):
    """{group: (sequences, logprobs | None)} for the query groups present, through the K|V-cached session or the re-run path.
    stream: a SampleStream (after begin_call) -> sampled decoding (beam 1) under `sampling` (a Sampling or None). constraints: a
    Constraints or None, for every mode; candidates: an AnswerSet fitted to the b rows (for_rows) or None. pool: (n_best,
    early_stopping[, num_beam_groups, diversity_penalty]) -> the beam search is decode_beam_pool and a group's entry its (seqs, rank,
    logprob, length[, beam group])"""
    c, a = constraints, candidates
    prompt = _prompt_rows(model, prompt, b)
    if stream is not None:
        beam = 1
    out = {}
    sess = _batch_session(model, b, beam, kv_layers, prompt, max_len, session)
    for g in ("tv", "tva", "ta"):
        if g not in groups:
            continue
        source = _group_source(sess, model, g, b, kv_layers, ranges, prompt)
        if stream is not None:
            out[g] = decode_sample(source, b, max_len, stream, sampling, c, a)
        elif pool is not None and beam > 1:
            out[g] = decode_beam_pool(source, b, beam, max_len, c, a, *pool)
        else:
            out[g] = (decode_beam(source, b, beam, max_len, c, a), None) if beam > 1 else decode_greedy(source, b, max_len, c, a)
    return out


def _prompt_rows(model, prompt, b):
    """prompt: 'caption' (-> the task prompt's b rows when the model uses one, else None) or host rows [b, L] as they are (QA: the questions)"""
    if isinstance(prompt, str):
        return model.get_task_prompt(PROMPTS[prompt], b) if model.use_task_prompt else None
    return prompt


def _batch_session(model, b, beam, kv_layers, prompt, max_len, make):
    """the K|V-cached session of a batch, holding the clips' K|V (make: `session`, the model's kept one of the geometry, or DecodeSession,
    the caller's own), or None: VALOR_KV_CACHE=0 and a cross-attention block per modality (bert.py:459-496) take the re-run path"""
    if not kv_cache_enabled() or isinstance(kv_layers, _BlockKV):
        return None
    sess = make(model, b, beam, 0 if prompt is None else prompt.shape[1], max_len, kv_layers)
    sess.begin_batch(kv_layers)
    return sess


def _group_source(sess, model, g, b, kv_layers, ranges, prompt):
    """the step source of query group g at its first step: the batch's session, reset, or a re-run source"""
    if sess is None:
        return _Rerun(_Stepper(model, g, kv_layers, ranges, prompt, b))
    sess.begin_group(ranges[g] if kv_layers is not None else None, prompt)
    return sess


def encode_for_generation(model, batch, groups):
    """The encoder half of generate_cap (pretrain.py:916-936): -> (batch size, per-layer K|V of the video/audio tokens, group key ranges)"""
    model.stage.begin_step()
    alltasks = "".join(groups)
    video_output = model.forward_video_encoder(batch["video_pixels"]) if "v" in alltasks else None
    audio_output = model.forward_audio_encoder(batch["audio_spectrograms"]) if "a" in alltasks else None
    b = (video_output if video_output is not None else audio_output).shape[0]
    kv_layers, ranges = model.cross_inputs(video_output, audio_output)
    return b, kv_layers, ranges


def stepper(model, group, b, kv_layers, ranges, prompt="caption"):
    """the per-step logits function of one query group ('tv' | 'tva' | 'ta'): stepper(...).logits(tokens so far or None, rows).
    prompt: 'caption' (the task prompt when the model uses one) or a host [b, L] tensor of prompt rows (QA: the questions)."""
    return _Stepper(model, group, kv_layers, ranges, _prompt_rows(model, prompt, b), b)


def _sample_stream(model, seed):
    return (sampler_of(model) if seed is None else SampleStream(seed)).begin_call()


def _repeat_clips(model, kv_layers, b, n):
    """every clip's per-layer K|V rows n times (n: an int, or one count per clip: generate_qa's sample_num), clip-major (rows
    i * n .. i * n + n - 1 are clip i): one row gather per layer"""
    if kv_layers is None:
        return None
    idx = model._dev(torch.arange(b, dtype=torch.long).repeat_interleave(n if isinstance(n, int) else torch.tensor(n, dtype=torch.long)))
    rows_of = lambda kvs: None if kvs is None else [ops.gather_rows(kv.reshape(b, -1), idx).view(idx.numel(), *kv.shape[1:]) for kv in kvs]
    return _BlockKV(rows_of(kv_layers.v), rows_of(kv_layers.a)) if isinstance(kv_layers, _BlockKV) else rows_of(kv_layers)


def _constraints_of(model, repetition_penalty, no_repeat_ngram_size, min_length, suppress_tokens, length_penalty):
    """the Constraints of a generate_* call: an argument that is None takes the model's option generation_<name> (absent: off)"""
    from .model.valor import _opt
    pick = lambda v, name, default: _opt(model.opts, "generation_" + name, default) if v is None else v
    return Constraints(pick(repetition_penalty, "repetition_penalty", 1.0), pick(no_repeat_ngram_size, "no_repeat_ngram_size", 0),
                       pick(min_length, "min_length", 0), pick(suppress_tokens, "suppress_tokens", ()),
                       pick(length_penalty, "length_penalty", 0.0))


def _sampling_of(model, temperature, top_k, top_p):
    from .model.valor import _opt
    return Sampling(_opt(model.opts, "sample_temperature", 1.0) if temperature is None else temperature,
                    _opt(model.opts, "sample_top_k", 0) if top_k is None else top_k,
                    _opt(model.opts, "sample_top_p", 1.0) if top_p is None else top_p)


def _resolve(who, model, mode, beam, max_generation_len, sample_only, controls, candidates):
    """what a generate_* call makes of its arguments -> (Sampling | None, Constraints, beam width, max_len, AnswerSet | None). who: the
    caller's name, for the error texts; beam: the width when mode is None; sample_only: {name: value} of the arguments that need
    mode='sample' (None: not given), temperature / top_k / top_p first; controls: the five arguments of _constraints_of"""
    if mode not in (None, "greedy", "sample"):
        raise ValueError(f"{who}: mode {mode!r} (None, 'greedy' or 'sample')")
    sampling = None
    if mode == "sample":
        sampling = _sampling_of(model, sample_only["temperature"], sample_only["top_k"], sample_only["top_p"])
    elif any(v is not None for v in sample_only.values()):
        raise ValueError(f"{who}: {' / '.join(sample_only)} need mode='sample'")
    constraints = _constraints_of(model, *controls)
    max_len = model.max_generation_len if max_generation_len is None else max_generation_len
    return sampling, constraints, beam if mode is None else 1, max_len, _check_candidates(model, candidates, constraints, max_len)


def _named(name, res, logprobs):
    """the result of a generate_* call from _decode_groups': name + 't_v' | 't_va' | 't_a' per group, and with `logprobs` 'logprobs_*'
    beside them where the decoder gave some (beam search gives none)"""
    out = {}
    for g, (seq, lp) in res.items():
        key = {"tv": "t_v", "tva": "t_va", "ta": "t_a"}[g]
        out[name + key] = seq
        if logprobs and lp is not None:
            out["logprobs_" + key] = lp
    return out


def _named_pool(name, res):
    """the result of a generate_* call under the pool search: name + key [b * n, L] clip-major (rows i * n .. i * n + n - 1 are the n
    best of clip i, best first), 'sequence_scores_' + key (the rank scores) and 'sequence_logprobs_' + key (the summed logP) [b * n];
    under beam groups 'sequence_groups_' + key besides (int64 [b * n]: the beam group of each hypothesis, GroupPoolState.result's order)"""
    out = {}
    for g, (seqs, rank, logprob, _, *group) in res.items():
        key = {"tv": "t_v", "tva": "t_va", "ta": "t_a"}[g]
        out[name + key] = seqs.reshape(-1, seqs.shape[-1])
        out["sequence_scores_" + key] = rank.reshape(-1)
        out["sequence_logprobs_" + key] = logprob.reshape(-1)
        if group:
            out["sequence_groups_" + key] = group[0].reshape(-1)
    return out


def _beam_groups(who, model, rule, beam, num_beam_groups, diversity_penalty, searching=True):
    """the beam groups of a generate_* call -> (num_beam_groups, diversity_penalty). None: the model's options
    generation_num_beam_groups (absent: 1) / generation_diversity_penalty (absent: 0.0). rule: _beam_rule's; searching: the call runs
    a beam search (mode None and a beam above 1). Groups or a penalty without the pool rule raise ValueError: GIVEN, with any call; from
    the model's options, with a call that searches under the reference rule (num_beam_groups=1, diversity_penalty=0.0 GIVEN switch
    them off for that call). To a call that runs no beam search the options simply do not apply, as generation_beam_search."""
    from .model.valor import _opt
    G = _opt(model.opts, "generation_num_beam_groups", 1) if num_beam_groups is None else num_beam_groups
    lam = _opt(model.opts, "generation_diversity_penalty", 0.0) if diversity_penalty is None else diversity_penalty
    if rule != "pool":
        given = (num_beam_groups is not None and num_beam_groups != 1) or (diversity_penalty is not None and diversity_penalty != 0.0)
        if given or (searching and (G != 1 or lam != 0.0)):
            raise ValueError(f"{who}: num_beam_groups {G!r} / diversity_penalty {lam!r} need beam_search='pool'"
                             + ("" if given else " (the model's options ask for them; this call searches under the reference rule)"))
        return 1, 0.0
    _grouped(who, beam, G, lam)
    return int(G), float(lam)


BEAM_RULES = ("reference", "pool")


def _beam_rule(who, model, mode, beam, beam_search, early_stopping):
    """the beam-search rule of a generate_* call -> (rule, early_stopping). beam_search / early_stopping None: the model's options
    generation_beam_search (absent: 'reference') / generation_early_stopping (absent: False). beam_search='pool' GIVEN with a call that
    runs no beam search (mode 'greedy' / 'sample', beam 1) raises; the model's option simply does not apply to such a call."""
    from .model.valor import _opt
    rule = _opt(model.opts, "generation_beam_search", "reference") if beam_search is None else beam_search
    if rule not in BEAM_RULES:
        raise ValueError(f"{who}: beam_search {rule!r} ('reference' or 'pool')")
    searching = mode is None and beam > 1
    if beam_search == "pool" and not searching:
        raise ValueError(f"{who}: beam_search='pool' needs a beam search (mode None and a beam above 1; got mode {mode!r}, beam {beam})")
    if not searching:
        rule = "reference"
    if early_stopping is not None and rule != "pool":
        raise ValueError(f"{who}: early_stopping needs beam_search='pool'")
    early = _opt(model.opts, "generation_early_stopping", False) if early_stopping is None else early_stopping
    return rule, bool(early)


@torch.no_grad()
def generate_cap(model, batch, groups, beam_size=None, max_generation_len=None, mode=None, seed=None, temperature=None, top_k=None,
                 top_p=None, num_return_sequences=1, repetition_penalty=None, no_repeat_ngram_size=None, min_length=None,
                 suppress_tokens=None, length_penalty=None, candidates=None, beam_search=None, early_stopping=None, num_beam_groups=None,
                 diversity_penalty=None):
    """VALOR.generate_cap, model/pretrain.py:914-985 -> {'generated_sequences_t_v' | '_t_va' | '_t_a' (+ 'logprobs_*' when greedy or
    sampled)}. mode: None (beam search when beam_size > 1, else greedy), 'greedy' (whatever beam_size says) or 'sample' (decode_greedy's
    sample mode, :1007-1011: a draw from softmax(logits) per step, logprobs_* = the logP of the draws). seed: the sampled draws' seed
    (None: the model's own SampleStream, seeded from opts.seed, advances one call).
    mode 'sample' only: temperature / top_k / top_p filter the distribution of every step (Sampling; None: the model's options
    sample_temperature / sample_top_k / sample_top_p, absent = off; logprobs_* are then the logP under the filtered distribution), and
    num_return_sequences = n draws n captions per clip: the encoders and the K|V projections run once per clip, the decoder runs b * n
    rows, and every output is [b * n, L] clip-major (rows i * n .. i * n + n - 1 belong to clip i).
    Every mode: repetition_penalty / no_repeat_ngram_size / min_length / suppress_tokens (Constraints; None: the model's options
    generation_<name>, absent = off) rewrite each step's logits on the device before the selection -- before temperature / top-k / top-p
    too, and the log-probabilities are those of what is left; length_penalty ranks the final hypotheses of a beam search.
    candidates: an AnswerSet (or a plain list of token lists: one shared set) -> every mode decodes INSIDE the set (one valor_trie_constrain
    launch per step): each output row is one of the candidates, AnswerSet.index_of names it; a per-sample set has one entry per clip
    (num_return_sequences rows read their clip's entry) or one per output row. It excludes the logits rules above (ValueError);
    length_penalty stays. In sample mode the logprobs are those of the masked row: a column outside the set has mass exactly 0.
    beam_search: None (the model's option generation_beam_search, absent = 'reference'), 'reference' (decode_beam: the reference's rule,
    unchanged) or 'pool' (decode_beam_pool: finished hypotheses leave the beam for a pool, length_penalty ranks while the search runs,
    the loop leaves early; early_stopping, None = the option generation_early_stopping: a sample stops once its pool is full). Under
    'pool', num_return_sequences = n <= beam_size returns the n best hypotheses of every clip: the outputs are [b * n, L] clip-major,
    best first, and 'sequence_scores_*' (logP * length^-length_penalty) / 'sequence_logprobs_*' (logP) [b * n] come beside them.
    beam_search='pool' with mode 'greedy' / 'sample' or beam 1 raises ValueError.
    num_beam_groups = G / diversity_penalty (None: the model's options generation_num_beam_groups, absent = 1, and
    generation_diversity_penalty, absent = 0.0), under 'pool' only: diverse beam search. The beam is G groups of beam_size / G, searched
    one after another inside every step; a later group pays diversity_penalty for every earlier group's slot that has just taken the
    same word (decode_beam_pool). The n returned are ordered by place within their group, then by score: the first G are one hypothesis
    per group, and 'sequence_groups_*' (int64 [b * n]) names the group of each. The penalty steers the selection only;
    'sequence_scores_*' / 'sequence_logprobs_*' stay true (length-ranked) log-probabilities. G not dividing beam_size, a negative or
    non-finite penalty, a penalty with one group, groups without beam_search='pool' raise ValueError."""
    n = int(num_return_sequences)
    if n != num_return_sequences or n < 1:
        raise ValueError(f"generate_cap: num_return_sequences {num_return_sequences!r} must be an integer >= 1")
    width = model.beam_size if beam_size is None else beam_size
    rule, early = _beam_rule("generate_cap", model, mode, width, beam_search, early_stopping)
    sampling, constraints, beam, max_len, aset = _resolve(
        "generate_cap", model, mode, width, max_generation_len,
        dict(temperature=temperature, top_k=top_k, top_p=top_p, num_return_sequences=None if n == 1 or rule == "pool" else n),
        (repetition_penalty, no_repeat_ngram_size, min_length, suppress_tokens, length_penalty), candidates)
    if rule == "pool":
        _check_pool("generate_cap", 0, beam, max_len, n)
    groups_of = _beam_groups("generate_cap", model, rule, beam, num_beam_groups, diversity_penalty, mode is None and beam > 1)
    was_training = model.training
    model.eval()
    try:
        b, kv_layers, ranges = encode_for_generation(model, batch, groups)
        if rule == "pool":
            if aset is not None:
                aset = aset.for_rows(b)
            res = _decode_groups(model, groups, b, kv_layers, ranges, "caption", beam, max_len, None, None, constraints, aset,
                                 (n, early) + groups_of)
            return _named_pool("generated_sequences_", res)
        if n > 1:
            kv_layers = _repeat_clips(model, kv_layers, b, n)
            b *= n
        if aset is not None:
            aset = aset.for_rows(b)
        stream = _sample_stream(model, seed) if mode == "sample" else None
        res = _decode_groups(model, groups, b, kv_layers, ranges, "caption", beam, max_len, stream, sampling, constraints, aset)
        return _named("generated_sequences_", res, True)
    finally:
        model.train(was_training)


@torch.no_grad()
def generate_qa(model, batch, groups, prompt_cpu, beam_size=None, max_generation_len=None, mode=None, seed=None, temperature=None,
                top_k=None, top_p=None, repetition_penalty=None, no_repeat_ngram_size=None, min_length=None, suppress_tokens=None,
                length_penalty=None, candidates=None, beam_search=None, early_stopping=None, num_beam_groups=None, diversity_penalty=None):
    """VALOR.generate_qa, model/pretrain.py:1366-1459: the caption decoders with the question rows as the prompt ->
    {'generated_answers_t_v' | '_t_va' | '_t_a'}. mode, seed, temperature / top_k / top_p and the Constraints arguments are
    generate_cap's: None (beam search when beam_size_qa > 1, else greedy), 'greedy', or 'sample' -- one sampled answer per question, with
    'logprobs_*' (the logP of the draws) beside the answers; the question tokens are no part of the history the constraints read.
    sample_num[i] consecutive question rows belong to clip i (:1378-1390): the reference
    expands the [video | audio] token rows per question; here the per-layer K|V projections are computed once per CLIP and their rows
    gathered per question (valor_gather_rows), so the projection GEMMs do not grow with the question count.
    candidates: generate_cap's -- closed-vocabulary QA: the answer is always one of the candidates (AnswerSet.index_of). A per-sample set
    has one entry per question row, or one per clip (its sample_num question rows read it).
    beam_search / early_stopping: generate_cap's; under 'pool' the best hypothesis is the answer and 'sequence_scores_*' /
    'sequence_logprobs_*' come beside it. num_beam_groups / diversity_penalty: generate_cap's (the answer is the overall best of the
    groups, 'sequence_groups_*' names its group)."""
    # the reference switches to beam search when beam_size_qa > 1 but decode_beam always searches with self.beam_size, task 'qa'
    # included (pretrain.py:1061): beam_size_qa is the switch, beam_size the width
    width = (model.beam_size if model.beam_size_qa > 1 else 1) if beam_size is None else beam_size
    rule, early = _beam_rule("generate_qa", model, mode, width, beam_search, early_stopping)
    sampling, constraints, beam, max_len, aset = _resolve(
        "generate_qa", model, mode, width, max_generation_len, dict(temperature=temperature, top_k=top_k, top_p=top_p),
        (repetition_penalty, no_repeat_ngram_size, min_length, suppress_tokens, length_penalty), candidates)
    if rule == "pool":
        _check_pool("generate_qa", 0, beam, max_len)
    groups_of = _beam_groups("generate_qa", model, rule, beam, num_beam_groups, diversity_penalty, mode is None and beam > 1)
    sample_num = [int(n) for n in batch.get("sample_num", [])]
    was_training = model.training
    model.eval()
    try:
        b, kv_layers, ranges = encode_for_generation(model, batch, groups)
        clips = b
        if any(n != 1 for n in sample_num):
            if len(sample_num) != b or sum(sample_num) != prompt_cpu.shape[0]:
                raise ValueError(f"sample_num {sample_num} does not describe {b} clips / {prompt_cpu.shape[0]} questions")
            kv_layers = _repeat_clips(model, kv_layers, b, sample_num)
            b = sum(sample_num)
        if aset is not None:
            aset = aset.for_rows(b, sample_num if b != clips and aset.n_roots == clips else None)
        stream = _sample_stream(model, seed) if mode == "sample" else None
        res = _decode_groups(model, groups, b, kv_layers, ranges, prompt_cpu, beam, max_len, stream, sampling, constraints, aset,
                             (1, early) + groups_of if rule == "pool" else None)
        if rule == "pool":
            return _named_pool("generated_answers_", res)
        return _named("generated_answers_", res, mode == "sample")
    finally:
        model.train(was_training)


def _forced_terms(logits, labels):
    """z[label] - lse(z) per fp32 row: the negated row loss of valor_xent_fwd (rows outside the session's padded buffer are copied once)"""
    return -_xent_rows(logits, labels)[0]


@torch.no_grad()
def score_candidates(model, batch, groups, candidates, prompt_cpu=None, max_rows=512):
    """The exact sequence log-probability of every candidate under the decoder -> {group: fp32 [b, Cmax]} on the device (slots beyond a
    sample's own count: -inf). For the candidate a_0 .. a_{L-1}, a_L = [SEP]:
        score = sum_{t = 0 .. L} (z_t[a_t] - lse(z_t)),   z_t = the decoding step's logits after the forced prefix a_<t,
    the terms added in fp32 in ascending t: what beam search assigns to that answer. candidates: an AnswerSet (shared: every sample scores
    the same C answers; per-sample: one entry per sample) or a plain list of token lists. prompt_cpu: the QA prompt rows [b, P] (host;
    model.qa_prompt of the questions), None: the caption prompt.
    Forced decoding on a DecodeSession of its own (beam 1, rows = sample x candidate through _repeat_clips, the prompt rows repeated the
    same way): every step's input is the previous forced token, a row past its end is fed [SEP] and left out of the sum, the per-step
    term is valor_xent_fwd's row loss with the forced tokens as labels. The candidates go in chunks of max(1, max_rows // b) per sample
    so that at most max(b, max_rows) decoder rows exist at once (a memory cap); every chunk has the same row count (the last is padded),
    so one session and one captured step serve the call. The session is the call's own: nothing stays in the model's pool. A model
    with a cross-attention block per modality (_BlockKV) and VALOR_KV_CACHE=0 take the re-run path (_Stepper), teacher-forced."""
    a = _answer_set(candidates)
    if a is None:
        raise ValueError("score_candidates: no candidates")
    a.check_vocab(model.spec.vocab)
    if a.max_len + 2 > model.spec.max_pos:
        raise ValueError(f"score_candidates: an answer of {a.max_len} tokens does not fit the decoder's {model.spec.max_pos} positions")
    was_training = model.training
    model.eval()
    try:
        b, kv_layers, ranges = encode_for_generation(model, batch, groups)
        sample_num = [int(n) for n in batch.get("sample_num", [])]
        if torch.is_tensor(prompt_cpu) and any(n != 1 for n in sample_num):      # several question rows per clip, as in generate_qa
            if len(sample_num) != b or sum(sample_num) != prompt_cpu.shape[0]:
                raise ValueError(f"sample_num {sample_num} does not describe {b} clips / {prompt_cpu.shape[0]} questions")
            kv_layers = _repeat_clips(model, kv_layers, b, sample_num)
            b = sum(sample_num)
        a = a.for_rows(b)
        dev = model.device
        per = [a.candidates[s % a.n_roots] for s in range(b)]
        Cmax = max(len(p) for p in per)
        chunk = min(Cmax, max(1, int(max_rows) // b))
        rows = b * chunk
        kv_rep = _repeat_clips(model, kv_layers, b, chunk)
        if isinstance(prompt_cpu, str) or prompt_cpu is None:
            prompt = _prompt_rows(model, prompt_cpu or "caption", rows)
        else:
            if prompt_cpu.shape[0] != b:
                raise ValueError(f"score_candidates: {prompt_cpu.shape[0]} prompt rows for {b} samples")
            prompt = prompt_cpu.repeat_interleave(chunk, 0)
        T = a.max_len + 1
        sess = _batch_session(model, rows, 1, kv_rep, prompt, T, DecodeSession)
        out = {g: torch.full((b, Cmax), -float("inf"), dtype=torch.float32, device=dev) for g in ("tv", "tva", "ta") if g in groups}
        for c0 in range(0, Cmax, chunk):
            forced = torch.full((rows, T), EOS, dtype=torch.long)
            length = torch.zeros(rows, dtype=torch.long)
            real = torch.zeros((b, chunk), dtype=torch.bool)
            for s in range(b):
                for j in range(chunk):
                    cand = per[s][c0 + j] if c0 + j < len(per[s]) else per[s][0]      # (a padding row repeats a real candidate)
                    forced[s * chunk + j, :len(cand)] = torch.tensor(cand, dtype=torch.long)
                    length[s * chunk + j] = len(cand)
                    real[s, j] = c0 + j < len(per[s])
            steps = int(length.max()) + 1
            forced_d, length_d, real_d = model._dev(forced), model._dev(length), model._dev(real)
            for g in out:
                score = torch.zeros(rows, dtype=torch.float32, device=dev)
                source = _group_source(sess, model, g, rows, kv_rep, ranges, prompt)
                for t in range(steps):
                    logits = source.step(None if t == 0 else forced_d[:, t - 1].contiguous())
                    term = _forced_terms(logits, forced_d[:, t].contiguous())
                    score = torch.where(length_d >= t, score + term, score)
                n = min(chunk, Cmax - c0)
                out[g][:, c0:c0 + n] = torch.where(real_d, score.view(b, chunk), -float("inf"))[:, :n]
        return out
    finally:
        model.train(was_training)


RANK_STORE_BYTES = 16 << 30              # rank_candidates' default cap on its self-attention slot store


def _rank_tree(model, g, b, kv_layers, ranges, prompt, a, max_rows):
    """rank_candidates for one query group and one sub-batch of b samples -> fp32 [b, C] on the device. kv_layers: the b clips' own
    per-layer K|V (rows are node-major, row = i * b + s: cross-attention reads clip row % b), prompt: their host prompt rows or None."""
    m, P_, dev, dt = model, model.P, model.device, model.dtype
    E, H, layers = m.spec.hidden, m.spec.heads, m.spec.layers
    e = "multimodal_encoder.embeddings."
    trie, lv = a.device(dev), a.levels(dev)
    N, D = a.n_nodes, lv.depth_max
    J = 1 if m.caption_type == "lm" else 2
    P = 0 if prompt is None else prompt.shape[1]
    Skv = P + D + 2                                                  # [prompt | text positions 0 .. D | the [MASK] behind the deepest]
    cn = min(lv.width, max(1, int(max_rows) // b))                   # nodes per launch of the layer stack
    max_r = cn * b
    tok0, mask0 = b * P, b * P + N * b                               # slots: P per sample, one per (node, sample), one [MASK] per chunk row
    slots = mask0 + (max_r if J == 2 else 0)
    store = torch.zeros((layers, slots, 2 * E), dtype=dt, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    cross = m._dev(torch.tensor([list(ranges[g])] * max_r, dtype=torch.int32)) if kv_layers is not None else None
    bmod = b if kv_layers is not None else 0
    s_idx = torch.arange(b, **i32)
    pm = None
    if P:                                                            # the prompt rows, once per sample: DecodeSession.begin_group's prefill
        pm = (1.0 - m._dev((prompt != 0).to(torch.float32))) * NEG                              # [b, P]: a zero-id key is masked
        pmask = pm[:, None, :].expand(b, P, P).contiguous()
        xp = m._bert_embed(m._dev(prompt), P, "prompt")

        def prefill(i, qkv):
            store[i, :tok0] = qkv[:, :, E:].reshape(tok0, 2 * E)
            return ops.self_attention(qkv, H, pmask, 0.0)
        m.bert_encoder(xp, pmask, kv_layers, cross[:b] if cross is not None else None, bmod, self_attn=prefill)
    Wd, Pe, Ty = P_[e + "word_embeddings.weight"], P_[e + "position_embeddings.weight"], P_[e + "token_type_embeddings.weight"]
    V = Wd.shape[0]
    logits_pad = torch.zeros((max_r, (V + 31) // 32 * 32), dtype=torch.float32, device=dev)
    node_score = torch.zeros(N * b, dtype=torch.float32, device=dev)          # the root's prefix score is 0
    final = torch.zeros(N * b, dtype=torch.float32, device=dev)
    col = torch.arange(Skv, device=dev)
    prompt_keys = (s_idx[:, None] * P + torch.arange(P, **i32)[None, :]) if P else None        # [b, P]
    for d in range(D + 1):
        for p0 in range(lv.level_ptr[d], lv.level_ptr[d + 1], cn):
            nodes = lv.order[p0:min(p0 + cn, lv.level_ptr[d + 1])].contiguous()
            c = nodes.numel()
            rows = c * b
            nl = nodes.long()
            # BertEmbeddings (bert.py:190-218) of the node's token at position d and of [MASK] at d + 1: DecodeSession._body's arithmetic
            ids = torch.full((rows, J), MASK, dtype=torch.int64, device=dev)
            ids[:, 0] = lv.token[nl].long().repeat_interleave(b)
            pos = torch.arange(d, d + J, device=dev)
            x = (Wd[ids].float() + Pe[pos].float()[None] + Ty[0].float()).to(dt)
            x = ops.layer_norm(x, P_[e + "LayerNorm.weight"], P_[e + "LayerNorm.bias"], 1e-12)
            # the key table: [the sample's prompt slots | the ancestors' and the row's own token slot | its [MASK] slot | slot 0, masked]
            anc = lv.anc[nl]                                                                     # [c, D + 1]
            table = torch.zeros((c, b, Skv), **i32)
            if P:
                table[:, :, :P] = prompt_keys[None]
            table[:, :, P:P + D + 1] = torch.where(anc[:, None, :] >= 0, tok0 + anc[:, None, :] * b + s_idx[None, :, None], 0)
            own = (tok0 + nodes[:, None] * b + s_idx[None, :]).reshape(rows, 1).long()
            new_slots = own
            if J == 2:
                mslot = mask0 + torch.arange(rows, **i32)
                table[:, :, P + d + 1] = mslot.view(c, b)
                new_slots = torch.cat((own, mslot.long()[:, None]), dim=1)
            new_slots = new_slots.reshape(-1)
            table = table.view(rows, Skv)
            amask = torch.where(col <= P + d, 0.0, NEG).to(torch.float32).expand(c, b, 1, Skv).repeat(1, 1, J, 1)
            if P:
                amask[:, :, :, :P] = pm[None, :, None, :]
            if J == 2:
                amask[:, :, 1, P + d + 1] = 0.0
            amask = amask.view(rows, J, Skv)

            def self_attn(i, qkv):
                st = store[i]
                st.index_copy_(0, new_slots, qkv[:, :, E:].reshape(rows * J, 2 * E))
                k = torch.as_strided(st, (slots, Skv, E), (2 * E, 0, 1), st.storage_offset())      # flat slots: the table names the row
                v = torch.as_strided(st, (slots, Skv, E), (2 * E, 0, 1), st.storage_offset() + E)
                return K.attn_decode(qkv[:, :, :E], k, v, H, mask=amask, key_row=table, scale=0.125)
            hidden = m.bert_encoder(x, None, kv_layers, cross[:rows] if cross is not None else None, bmod, self_attn=self_attn)
            h = m.cls_transform(hidden[:, J - 1].contiguous())
            logits = logits_pad[:rows, :V]
            K.gemm(h, Wd, bias=P_["cls.decoder.bias"], out=logits, out_dtype=torch.float32, policy=K.infer_policy())
            K.trie_score_level(logits, nodes, b, EOS, trie, node_score, final)
    return final.view(N, b)[lv.cand_node].t().contiguous()


@torch.no_grad()
def rank_candidates(model, batch, groups, candidates, prompt_cpu=None, k=None, max_rows=8192, max_store_bytes=RANK_STORE_BYTES):
    """The exact sequence log-probability of EVERY answer of a shared closed set, for every sample: score_candidates' inputs and output
    ({group: fp32 [b, C]} on the device, duplicates carry equal scores; sample_num, the caption prompt, 'unimlm' and 'lm' as there), by
    level-batched trie scoring: one decoder row per trie NODE and sample instead of one per (candidate, step). A node's logits row
    scores all its children and its own end-of-answer term in one valor_trie_score_level launch, prefixes are computed once, and the
    whole set is ranked in depth + 1 passes over the layer stack (b * n_nodes rows in all, against b * C * (Lmax + 1)).
    k (1 .. min(256, C)): -> {group: (values fp32 [b, k], indices int64 [b, k])} through valor_topk_rows: scores descending, equal
    scores in index order (the lowest duplicate first).
    The rows of a pass are node-major (row = i * b + s), so cross-attention reads clip row % b: the clips' K|V are not copied.
    Self-attention K|V lives in a flat slot store [layers, slots, 2E]: P prompt slots per sample (one prefill, zero-id keys masked),
    one token slot per (node, sample), one transient [MASK] slot per row of the current chunk ('unimlm'); an int32 key table
    [rows, P + depth + 2] names, per row, its sample's prompt slots, its ancestors' token slots, its own, and its [MASK] slot, and
    valor_attn_decode_fwd reads the keys where they were written (zero key row stride): nothing moves from parent to child.
    max_rows: a level wider than max_rows // b nodes runs in chunks of nodes; max_store_bytes: when the slot store of b samples
    would be larger, the samples go in sub-batches (halved until it fits). Chunking changes a score only through the GEMM kernel the
    row count selects. Issued eagerly: depth + 1 wide passes, nothing to capture. Nothing stays in the model's session pool; the
    model is in eval mode for the call and gets its mode back.
    A per-sample set raises ValueError: score_candidates is the tool for a handful of choices per question. A model with a
    cross-attention block per modality (_BlockKV) and VALOR_KV_CACHE=0 have no tree pass: they delegate to score_candidates."""
    a = _answer_set(candidates)
    if a is None:
        raise ValueError("rank_candidates: no candidates")
    if a.per_sample:
        raise ValueError("rank_candidates: a per-sample set has no shared trie to batch by level; score_candidates scores a handful of "
                         "choices per question")
    C = a.counts[0]
    if k is not None and (int(k) != k or not 1 <= k <= min(256, C)):
        raise ValueError(f"rank_candidates: k = {k!r} outside 1 .. min(256, {C} candidates) (valor_topk_rows)")
    a.check_vocab(model.spec.vocab)
    if a.max_len + 2 > model.spec.max_pos:
        raise ValueError(f"rank_candidates: an answer of {a.max_len} tokens does not fit the decoder's {model.spec.max_pos} positions")

    def best(out):
        if k is None:
            return out
        from .search import topk_rows
        return {g: topk_rows(sc.contiguous(), int(k)) for g, sc in out.items()}
    if not kv_cache_enabled() or model.spec.cross_attn_type != "va_concate":
        return best(score_candidates(model, batch, groups, a, prompt_cpu=prompt_cpu))
    was_training = model.training
    model.eval()
    try:
        b, kv_layers, ranges = encode_for_generation(model, batch, groups)
        sample_num = [int(n) for n in batch.get("sample_num", [])]
        if torch.is_tensor(prompt_cpu) and any(n != 1 for n in sample_num):      # several question rows per clip, as in generate_qa
            if len(sample_num) != b or sum(sample_num) != prompt_cpu.shape[0]:
                raise ValueError(f"sample_num {sample_num} does not describe {b} clips / {prompt_cpu.shape[0]} questions")
            kv_layers = _repeat_clips(model, kv_layers, b, sample_num)
            b = sum(sample_num)
        if isinstance(prompt_cpu, str) or prompt_cpu is None:
            prompt = _prompt_rows(model, prompt_cpu or "caption", b)
        else:
            if prompt_cpu.shape[0] != b:
                raise ValueError(f"rank_candidates: {prompt_cpu.shape[0]} prompt rows for {b} samples")
            prompt = prompt_cpu
        lv = a.levels()
        P = 0 if prompt is None else prompt.shape[1]
        if P + lv.depth_max + 2 > 256:
            raise ValueError(f"rank_candidates: {P} prompt slots + {lv.depth_max + 2} text slots exceed the 256 keys of valor_attn_decode_fwd")
        J = 1 if model.caption_type == "lm" else 2
        slot_bytes = model.spec.layers * 2 * model.spec.hidden * torch.empty((), dtype=model.dtype).element_size()
        need = lambda n: (n * (P + a.n_nodes) + (J - 1) * min(lv.width, max(1, int(max_rows) // n)) * n) * slot_bytes
        bs = b
        while bs > 1 and need(bs) > max_store_bytes:
            bs = (bs + 1) // 2
        out = {g: torch.empty((b, C), dtype=torch.float32, device=model.device) for g in ("tv", "tva", "ta") if g in groups}
        for s0 in range(0, b, bs):
            s1 = min(b, s0 + bs)
            kv_sub = kv_layers if kv_layers is None or (s0 == 0 and s1 == b) else [kv[s0:s1] for kv in kv_layers]
            for g in out:
                out[g][s0:s1] = _rank_tree(model, g, s1 - s0, kv_sub, ranges, None if prompt is None else prompt[s0:s1], a, max_rows)
        return best(out)
    finally:
        model.train(was_training)
