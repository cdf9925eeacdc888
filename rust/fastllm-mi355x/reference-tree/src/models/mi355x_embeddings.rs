//! MI355X (gfx950) backend for the embeddings path: `impl EmbeddingModel` (src/models/embeddings.rs:17-38) on top of
//! `fastllm_mi355x::Encoder`.  A new file for the FastLLM tree, NOT wired in by `patches/0001-mi355x-backend.patch` yet: to use it,
//! add `pub mod mi355x_embeddings;` to src/models/mod.rs and build a `Mi355xEmbeddingModel` at the place that builds `MiniLMModel`
//! today, out of the pieces that place already has.
//!
//! This file does not fetch, parse or tokenize-configure anything.  Everything the host side of the reference prepares -- the
//! `Tokenizer`, the parsed `BertConfig`, the `do_lower_case` flag of the sentence-transformers config and the checkpoint's tensors
//! -- is handed to `from_parts`; what happens here is the marshalling of those tensors into the library and the trait methods.
//! On the GPU: the encoder forward, mean pooling and L2 normalisation; `embed_many` sends many texts in one packed call, which a
//! one-text-at-a-time CPU forward cannot do.  The forward options are pinned to what the reference computes: tanh-form GELU
//! (candle's `Tensor::gelu`) and no token-type row.
use std::collections::HashMap;

use anyhow::{anyhow, Result};
use candle_core::{DType, Device, Tensor};
use fastllm_mi355x as mi;
use tokenizers::Tokenizer;

use super::embeddings::{BertConfig, EmbeddingModel, EmbeddingOutput};

pub struct Mi355xEmbeddingModel {
    tokenizer: Tokenizer,
    encoder: mi::Encoder,
    label: String,
    lower: bool,
}

/// One checkpoint tensor as the library wants it: dtype tag, shape, little-endian bytes.
struct Marshalled {
    name: String,
    dtype: mi::DType,
    shape: Vec<usize>,
    bytes: Vec<u8>,
}

fn marshal(name: String, tensor: &Tensor) -> Result<Marshalled> {
    let host = tensor.to_device(&Device::Cpu)?.contiguous()?;
    let shape = host.dims().to_vec();
    let flat = host.flatten_all()?;
    let mut bytes = Vec::with_capacity(flat.elem_count() * 4);
    let dtype = match host.dtype() {
        DType::F32 => {
            for x in flat.to_vec1::<f32>()? {
                bytes.extend_from_slice(&x.to_le_bytes());
            }
            mi::DType::F32
        }
        DType::BF16 => {
            for x in flat.to_vec1::<half::bf16>()? {
                bytes.extend_from_slice(&x.to_bits().to_le_bytes());
            }
            mi::DType::BF16
        }
        DType::F16 => {
            for x in flat.to_vec1::<half::f16>()? {
                bytes.extend_from_slice(&x.to_bits().to_le_bytes());
            }
            mi::DType::F16
        }
        other => return Err(anyhow!("MI355X encoder: tensor {} is {:?}; only f32, bf16 and f16 can be handed over", name, other)),
    };
    Ok(Marshalled { name, dtype, shape, bytes })
}

impl Mi355xEmbeddingModel {
    /// `label` is what `model_id()` reports.  `tensors` are the checkpoint's, under their own names (no `bert.` prefix); they are
    /// consumed, so the host copies are freed one by one as they are marshalled.  `compute`: `mi::DType::F32` gives the reference's
    /// fp32 results to fp32 rounding, `mi::DType::BF16` is the fast mode.  The GPU is `FASTLLM_MI355X_DEVICE` (default 0), as for
    /// the decoder backend.
    pub fn from_parts(
        label: &str,
        tokenizer: Tokenizer,
        config: &BertConfig,
        do_lower_case: bool,
        tensors: HashMap<String, Tensor>,
        compute: mi::DType,
    ) -> Result<Self> {
        let mut staged = Vec::with_capacity(tensors.len());
        for (name, tensor) in tensors {
            staged.push(marshal(name, &tensor)?);
        }
        let views: Vec<mi::TensorView<'_>> = staged.iter().map(|m| mi::TensorView::host(&m.name, m.dtype, &m.shape, &m.bytes)).collect();
        let cfg = mi::EncoderConfig {
            hidden_size: config.hidden_size,
            num_attention_heads: config.num_attention_heads,
            num_hidden_layers: config.num_hidden_layers,
            intermediate_size: config.intermediate_size,
            max_position_embeddings: config.max_position_embeddings,
            layer_norm_eps: config.layer_norm_eps,
            vocab_size: tokenizer.get_vocab_size(false),
            activation: mi::Activation::GeluTanh,
            add_token_type0: false,
            max_batch_tokens: 0,
        };
        let gpu = std::env::var("FASTLLM_MI355X_DEVICE").ok().and_then(|s| s.parse::<i32>().ok()).unwrap_or(0);
        let encoder = mi::Encoder::new(&cfg, &views, compute, gpu).map_err(|e| anyhow!("MI355X encoder for {} could not be built: {}", label, e))?;
        Ok(Self { tokenizer, encoder, label: label.to_owned(), lower: do_lower_case })
    }

    /// Token ids of one text, special tokens included, after the optional lower-casing.
    fn ids_of(&self, text: &str) -> Result<Vec<u32>> {
        let folded;
        let input = if self.lower {
            folded = text.to_lowercase();
            folded.as_str()
        } else {
            text
        };
        match self.tokenizer.encode(input, true) {
            Ok(enc) => Ok(enc.get_ids().to_vec()),
            Err(e) => Err(anyhow!("MI355X encoder: the tokenizer rejected the text: {}", e)),
        }
    }

    fn output(&self, embeddings: Vec<f32>, token_count: usize) -> EmbeddingOutput {
        EmbeddingOutput { embeddings, model: self.label.clone(), token_count }
    }

    /// Many texts in one packed GPU call; result `i` is what `embed(texts[i])` returns.
    pub fn embed_many(&self, texts: &[&str]) -> Result<Vec<EmbeddingOutput>> {
        let mut ids = Vec::with_capacity(texts.len());
        for t in texts {
            ids.push(self.ids_of(t)?);
        }
        let slices: Vec<&[u32]> = ids.iter().map(Vec::as_slice).collect();
        let rows = self.encoder.embed(&slices).map_err(|e| anyhow!("MI355X encoder: {}", e))?;
        Ok(rows.into_iter().zip(ids.iter()).map(|(row, i)| self.output(row, i.len())).collect())
    }
}

impl EmbeddingModel for Mi355xEmbeddingModel {
    fn embed(&self, text: &str) -> Result<EmbeddingOutput> {
        let ids = self.ids_of(text)?;
        let row = self
            .encoder
            .embed(&[ids.as_slice()])
            .map_err(|e| anyhow!("MI355X encoder: {}", e))?
            .pop()
            .ok_or_else(|| anyhow!("MI355X encoder: no embedding came back"))?;
        Ok(self.output(row, ids.len()))
    }

    fn model_id(&self) -> String {
        self.label.clone()
    }

    fn embedding_size(&self) -> usize {
        self.encoder.embedding_size()
    }
}
