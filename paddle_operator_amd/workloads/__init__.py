"""Workloads a PaddleJob launches through ``pdo-launch`` (BASELINE configs).

* ``gpt2``      — GPT-2(-medium) LM training, collective DP (config 4)
* ``resnet50``  — ResNet-50 image classification, collective DP (configs 2, 3, 5)
* ``wide_deep`` — Wide & Deep CTR: parameter-server mode on CPU (config 1) when the job
  has pserver endpoints; in a Collective or Single job ``workloads.ctr.CTRTrainer`` on
  the GPU — fused sparse lookup and deterministic sparse Adagrad (``csrc/hip/ctr.hip``),
  replicated tables, the dense tower on torch
* ``deepfm``    — DeepFM CTR (FM + deep over the same tables), both ways as ``wide_deep``
* ``noop``      — bootstrap + readiness only (launch-latency measurement)

Every workload uses synthetic data of the benchmark's shape and random-init
weights (no network / datasets in this environment).
"""
WORKLOADS = ("gpt2", "resnet50", "wide_deep", "deepfm", "noop")
