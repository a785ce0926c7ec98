#!/usr/bin/env python3
"""Distributed MNIST training — CLI-compatible with the reference ``main.py``.

    python main.py [--train_dir=/tmp/mnist_train] [--config=params.yaml]
    # data parallel (RCCL all-reduce over xGMI), one process per GPU:
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 main.py
    # parameter-server mode (reference semantics), e.g. 1 PS + 2 workers on one node:
    python main.py --job_name=ps     --task_id=0 --ps_hosts=localhost:2222 --worker_hosts=localhost:2223,localhost:2224
    python main.py --job_name=worker --task_id=0 --ps_hosts=localhost:2222 --worker_hosts=localhost:2223,localhost:2224
    python main.py --job_name=worker --task_id=1 --ps_hosts=localhost:2222 --worker_hosts=localhost:2223,localhost:2224

Reference flags (main.py:12-32): job_name, ps_hosts, worker_hosts, task_id,
train_dir, log_device_placement.  Hyper-parameters come from the parameter
manager (``--config`` YAML/JSON or ``MNISTX_PARAMS``), as DLI's
tf_parameter_mgr provided them; the extra flags below override it.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from distributed_tensorflow_ibm_mnist_amd.utils import flags  # noqa: E402

FLAGS = flags.FLAGS

# ---- reference flags (main.py:12-32)
flags.DEFINE_string("job_name", "", 'One of "ps", "worker"')
flags.DEFINE_string("ps_hosts", "", "Comma-separated list of hostname:port for the parameter server jobs.")
flags.DEFINE_string("worker_hosts", "", "Comma-separated list of hostname:port for the worker jobs.")
flags.DEFINE_integer("task_id", 0, "Task ID of the worker/replica running the training.")
flags.DEFINE_string("train_dir", "/tmp/mnist_train", "Directory where to write event logs and checkpoint.")
flags.DEFINE_boolean("log_device_placement", False, "Whether to log device placement.")

# ---- parameter manager (tf_parameter_mgr) source + overrides
flags.DEFINE_string("config", "", "YAML/JSON hyper-parameter file (the DLI job config replacement)")
flags.DEFINE_integer("max_steps", -1, "override getMaxSteps()")
flags.DEFINE_integer("test_interval", -1, "override getTestInterval()")
flags.DEFINE_integer("batch_size", -1, "override getTrainBatchSize() (per replica)")
flags.DEFINE_float("base_lr", -1, "override getBaseLearningRate()")
flags.DEFINE_float("lr_decay", -1, "override getLearningRateDecay()")
flags.DEFINE_string("optimizer", "", "override getOptimizer(): sgd | momentum | nesterov | adam | rmsprop | adagrad "
                    "| lars | lamb (the adaptive three: TF1 semantics and defaults; lars / lamb: layer-wise trust "
                    "ratios on momentum / adam; none of the five in parameter-server mode)")
flags.DEFINE_float("momentum", -1, "momentum for --optimizer=momentum|nesterov; with rmsprop, its momentum (default 0)")
flags.DEFINE_float("beta1", -1, "adam: override beta1 (0.9)")
flags.DEFINE_float("beta2", -1, "adam: override beta2 (0.999)")
flags.DEFINE_float("epsilon", -1, "adam / rmsprop: override epsilon (1e-8 / 1e-10)")
flags.DEFINE_float("rmsprop_decay", -1, "rmsprop: override the decay of the mean square (0.9)")
flags.DEFINE_float("adagrad_initial_accumulator", -1, "adagrad: override the accumulator's initial value (0.1)")
flags.DEFINE_float("clip_norm", -1, "clip the gradients by this global norm (tf.clip_by_global_norm) before any "
                   "rule's update; -1: unset (off unless the config sets it); not in parameter-server mode")
flags.DEFINE_float("lars_eta", -1, "lars: override the trust coefficient (0.001)")
flags.DEFINE_string("lr_schedule", "", "learning-rate schedule: staircase (default) | polynomial | cosine; the last two "
                    "decay from the end of the warmup to --lr_end at --lr_total_steps; not in parameter-server mode")
flags.DEFINE_integer("warmup_steps", -1, "linear warmup (step + 1) / warmup_steps in front of any schedule (0: none); "
                     "not in parameter-server mode")
flags.DEFINE_integer("lr_total_steps", -1, "polynomial | cosine: the step at which --lr_end is reached (max_steps)")
flags.DEFINE_float("lr_end", -1, "polynomial | cosine: the rate from --lr_total_steps on (0.0)")
flags.DEFINE_float("lr_power", -1, "polynomial: the exponent (1.0)")
flags.DEFINE_float("label_smoothing", -1, "train against (1 - eps) * onehot + eps / classes, 0 <= eps < 1 (0.0: hard "
                   "labels); the training cross_entropy / total_loss are the smoothed loss, every eval stays plain")
flags.DEFINE_float("dropout", -1, "drop rate 0 <= p < 1 on the hidden ReLU dense layers' outputs, training only (0.0: "
                   "off; -1: unset); masks from a counter-based RNG on the device; not in parameter-server mode")
flags.DEFINE_integer("dropout_seed", -1, "seed of the dropout masks (-1: unset, the run's --seed); rank r uses seed + r")
flags.DEFINE_integer("augment_shift", -1, "training images only: random translation of up to this many whole pixels, "
                     "0..8, independently in x and y (0: off; -1: unset)")
flags.DEFINE_float("augment_rotate", -1, "training images only: random rotation about the image centre of up to this "
                   "many degrees, 0..180 (0.0: off; -1: unset)")
flags.DEFINE_float("augment_scale", -1, "training images only: random zoom drawn from [1 - z, 1 + z), 0..0.5 (0.0: off; "
                   "-1: unset); any of the three on trains in --input_mode prep")
flags.DEFINE_integer("augment_seed", -1, "seed of the augmentation draws (-1: unset, the run's --seed); a draw is a "
                     "function of (seed, stream position), so a resumed run repeats it")
flags.DEFINE_float("augment_elastic_alpha", -1, "training images only: elastic distortion, the displacement scale in pixels "
                   "of the smoothed random field, 0..64 (0.0: off; -1: unset); on trains in --input_mode prep")
flags.DEFINE_float("augment_elastic_sigma", -1, "standard deviation in pixels of the Gaussian that smooths the elastic "
                   "field, 0.5..8 (-1: unset, 4.0); read only when augment_elastic_alpha > 0")
flags.DEFINE_float("mixup_alpha", -1, "training batches only: mixup of every entry with the entry at the flipped batch "
                   "position, the weight from Beta(a, a), 0.1..8 (0.0: off; -1: unset, the config's value or 0.0)")
flags.DEFINE_float("cutmix_alpha", -1, "training batches only: CutMix, a box of the partner pasted in, its area from "
                   "Beta(a, a), 0.1..8 (0.0: off; -1: unset); with mixup_alpha also set each entry takes one of the two")
flags.DEFINE_float("mix_prob", -1, "probability that a batch entry is mixed at all, 0..1 (-1: unset, 1.0)")
flags.DEFINE_string("distill_from", "", "knowledge distillation: the checkpoint directory of a frozen teacher whose "
                    "logits at a temperature become a soft target of the training loss ('': off)")
flags.DEFINE_string("distill_model", "", "the teacher's registry name (required with --distill_from); its input "
                    "channels, input size and class count must be the student's")
flags.DEFINE_float("distill_alpha", -1, "weight of the soft part: loss = (1 - a) CE + a T^2 KL(teacher || student), "
                   "0..1 (-1: unset, 0.5 with --distill_from)")
flags.DEFINE_float("distill_temperature", -1, "the temperature T > 0 of the teacher's and the student's softmax in "
                   "the soft part (-1: unset, 2.0)")
flags.DEFINE_integer("distill_use_ema", -1, "1: restore the teacher's ExponentialMovingAverage shadows (-1: unset, 0)")
flags.DEFINE_integer("mix_seed", -1, "seed of the mixing draws (-1: unset, the run's --seed); a draw is a pure function "
                     "of (seed, stream position), so a resumed run repeats it")
flags.DEFINE_string("train_data", "", "override getTrainData() (comma list: TFRecords, synthetic://, idx://, png://)")
flags.DEFINE_string("test_data", "", "override getTestData()")
flags.DEFINE_string("val_data", "", "override getValData()")

# ---- framework flags
flags.DEFINE_string("model", "reference_cnn", "reference_cnn | lenet5 | mlp")
flags.DEFINE_integer("in_channels", 3, "model input channels: 3 = DLI RGB records (reference), 1 = grayscale")
flags.DEFINE_string("impl", "hip", "hip = MI355X HIP kernels; torch = plain PyTorch (CPU path / baseline)")
flags.DEFINE_boolean("cpu", False, "force the CPU (torch impl, gloo)")
flags.DEFINE_string("precision", "bf16", "HIP compute precision: bf16 (bf16 operands, fp32 accumulate) | fp32 "
                    "(the reference's tf.float32: fp32 activations and fp32 MFMA)")
flags.DEFINE_integer("seed", 0, "random seed (weights, shuffling)")
flags.DEFINE_boolean("train_on_eval_split", False, "parity with the reference, which trains on getTestData() (Q1)")
flags.DEFINE_boolean("no_shard", False, "every DP rank reads the whole dataset in its own order (reference P3)")
flags.DEFINE_boolean("verbose_steps", False, "print 'training' + step on every step like the reference (Q11)")
flags.DEFINE_boolean("hip_graph", True, "capture the training step in a hipGraph (single GPU)")
flags.DEFINE_boolean("hip_graph_dp", False, "data parallel: also capture the step with its RCCL all-reduces "
                     "(rehearsed with one-rank RCCL and gloo ranks sharing a GPU; a real multi-GPU capture is "
                     "UNVERIFIED -- the eager DP path is the default)")
flags.DEFINE_float("bucket_mb", 0.125, "gradient all-reduce bucket cap (MB); every bucket but the last overlaps backward")
flags.DEFINE_boolean("fused_input", False, "HIP: first fused conv reads the uint8 dataset through the batch index")
flags.DEFINE_string("input_mode", "bf16", "HIP input path: bf16 | u8 (the first fused conv gathers the resident "
                    "training set, normalised once to bf16 / in the kernels from uint8) | prep (a per-step "
                    "gather+normalise kernel); models whose first layer cannot gather fall back to prep")
flags.DEFINE_float("save_checkpoint_secs", 600, "checkpoint every N seconds (TF default 600)")
flags.DEFINE_integer("save_checkpoint_steps", 0, "checkpoint every N steps (0: off)")
flags.DEFINE_integer("save_summaries_steps", 100, "loss/accuracy scalars every N steps")
flags.DEFINE_integer("log_step_count_steps", 100, "global_step/sec every N steps")
flags.DEFINE_integer("max_to_keep", 5, "checkpoints to keep")
flags.DEFINE_integer("nan_check_steps", -1, "NaN guard: read the device NaN flag every N steps, asynchronously "
                     "(a NaN at step k raises by step k + N); -1 = --log_step_count_steps (100 when that is 0)")
flags.DEFINE_integer("eval_examples", 10000, "examples per test-summary evaluation (0: whole split)")
flags.DEFINE_integer("monitor_device", 0, "1: the chief's train summaries (histograms, norms, gw_ratio) are reduced "
                     "on the GPU and only bucket counts and moments are copied to the host; 0: host numpy. CPU "
                     "executors always use the host path")
flags.DEFINE_integer("eval_metrics", 0, "1: every test summary also reports top-2 / top-3 accuracy, NLL, Brier score, "
                     "ECE / MCE, macro-F1 and per-class recall / precision (computed on the GPU for --impl=hip, by "
                     "the host reference otherwise) and appends a line to <train_dir>/log/eval_metrics.jsonl; 0: "
                     "loss and accuracy alone")
flags.DEFINE_string("ps_backend", "", "PS-mode data plane: '' (GPU: shm for PS shards up to 1 M parameters, e.g. "
                    "LeNet-5, ipc above, e.g. the reference CNN; CPU: host) | shm (CPU parameter server "
                    "serving a shared-memory segment natively; one host) | ipc (xGMI peer copies into a GPU PS) | "
                    "host / gloo (staged through host memory)")
flags.DEFINE_string("dp_backend", "", "DP transport override: '' (RCCL on GPU, gloo on CPU) | gloo (host-staged; "
                    "lets several ranks share one GPU for a rehearsal)")
flags.DEFINE_float("collective_timeout", 600.0, "process-group timeout (s): a hung peer fails the job")


def main(argv=None):
    # a PS / worker task with an adaptive optimizer, clip_norm, dropout, a warmup or a schedule other
    # than the staircase stops here, before torch is even imported
    from distributed_tensorflow_ibm_mnist_amd.utils import parameter_mgr
    parameter_mgr.configure_from_flags(FLAGS)
    parameter_mgr.check_ps_optimizer(FLAGS.job_name)
    parameter_mgr.check_ps_clip_norm(FLAGS.job_name)
    parameter_mgr.check_ps_lr_schedule(FLAGS.job_name)
    parameter_mgr.check_ps_dropout(FLAGS.job_name)
    if FLAGS.ps_hosts and FLAGS.job_name in ("ps", "worker") and "GPU_MAX_HW_QUEUES" not in os.environ:
        # PS mode only (data-parallel workers keep HIP's default queues, so the RCCL stream
        # does not share a queue with compute): PS tasks are often co-located on one GPU,
        # and one hardware queue per process keeps their queues from oversubscribing the
        # GPU's scheduler (0.21-0.25 ms per applied update vs 0.47-0.51 at the default 4,
        # profiles/r3/ps/).  Set before HIP starts; a value the user set is kept.
        os.environ["GPU_MAX_HW_QUEUES"] = os.environ.get("MNISTX_PS_HW_QUEUES", "1")
    from distributed_tensorflow_ibm_mnist_amd.train.trainer import train
    res = train(FLAGS)
    if res:
        print("result: " + " ".join(f"{k}={v:.6g}" if isinstance(v, float) else f"{k}={v}" for k, v in res.items()))
    return 0


if __name__ == "__main__":
    flags.run(main)
