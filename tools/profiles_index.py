#!/usr/bin/env python3
"""profiles/README.md = this table: file pattern -> one line -> where it is quoted.  `python tools/profiles_index.py` rewrites the README and
fails if a file under profiles/ matches no row (tests/test_api.py runs the check).  rNN = any round that has the file; the newest is the one quoted."""
import fnmatch
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
D, E = 'DESIGN', 'EXPERIMENTS'
ROWS = [
    # ---- the round's core set (tools/profile_round.sh)
    ('r0?_bench_line.json', 'python bench.py: the driver-visible line with every extra', f'{D} 7.1, 7.2'),
    ('r0?_bench_line_k20.json', 'bench.py --steps 20 --warmup 5 --no-extras: the driver\'s short shape', f'{D} 7.1'),
    ('r0?_bench_line_c4.json', 'bench.py --config c4: the 8192 x 4096 shard of BASELINE config 4', f'{D} 7.2'),
    ('r0?_bench_line_final.json|r0?_bench_line_live_pmc.json', 'further runs of the default line (round 4 / 5: final tree, first run with live PMC traffic)', f'{E} 5'),
    ('r0?_bench_line_2ranks_*.json|r0?_bench_line_?ranks_c?_shared.json', 'bench.py --gpus N with the ranks sharing one GPU: the launch paths of an 8-GPU lease', f'{D} 8'),
    ('r0?_strong_*ranks_one_gpu.json', '--scaling strong: one tensor cut over N ranks sharing the GPU', f'{D} 8'),
    ('r0?_strong_*_emulated_world_?.json', "--emulate-world M: rank 0's slice of an M-way cut alone on the GPU + the projected M-GPU figure", f'{D} 8'),
    ('r0?_bench_kernel_stats.csv', 'rocprofv3 --kernel-trace --stats over bench.py --no-extras: per-dispatch averages of the two kernels', f'{D} 7.1'),
    ('r0?_pmc_traffic.json|traffic_forward.json|r01_pmc_*_counter_collection.csv', 'PMC FETCH_SIZE (x2, gfx950) + WRITE_SIZE passes: HBM bytes per launch', f'{D} 7.1'),
    ('r0?_configs.json', 'every BASELINE config warm and cold: rocprofv3 per-dispatch durations + PMC traffic per phase', f'{D} 7.2'),
    ('r0?_roberta_base*.json|r01_roberta_readme_table.json', 'RoBERTa-base b128 x s128: vanilla, fewbit.GELU route, raw-operator route', f'{D} 7.2'),
    ('r0?_roberta_insitu.json|r0?_roberta_kernel_stats_*.csv', 'rocprofv3 kernel stats of the RoBERTa step: the few-bit kernels inside training', f'{D} 7.2'),
    ('r0?_hostcost.json|r0?_oplevel_graph.txt|r0?_wall_overhead.txt', 'host cost per operator call; hipGraph replay; wall-clock overhead of a 20-step region', f'{E} 5'),
    ('r0?_clock_transient_timeline.txt', 'step time against time since idle: the transient every settled figure waits out', f'{D} 7'),
    ('r0?_stream_bench_*MiB.txt', 'bare copy / read / write kernels and an empty kernel: the floors', f'{D} 7.1, 9'),
    ('r0?_fp32_ulp.json', 'ULP histogram of the fp32 GELU forward against the reference run and the exact value', f'{D} 6'),
    ('r0?_soak_fuzz.txt|r0?_sketch_soak_fuzz.txt|r06_dct_soak_fuzz.txt', 'one-off soak runs of the differential fuzz tests', f'{D} 6'),
    # ---- estimators of the randomized layers
    ('r0?_sketch_bench*.json', 'tools/sketch_bench.py: every estimator per shape against torch (round 6: settled, with the dct / dft columns; _torchfft_dct: before the DCT kernel existed)', f'{D} 7.3'),
    ('r0?_sketch_rocprof_*.txt', 'tools/profile_sketch.sh: rocprofv3 kernel durations (round 6: >= 200 settled dispatches) + PMC counters of the dense sketches', f'{D} 7.3'),
    ('r06_dct_rocprof_*.txt', 'tools/profile_dct.sh: settled kernel durations and PMC traffic of the sampled-DCT kernel pair', f'{D} 5, 7.3'),
    ('r06_dct_large_rows.txt', 'the kernel pair and the torch.fft formulation at 32768 and 65536 rows', f'{D} 7.3'),
    ('r06_convergence_demo_*.txt', 'a student MLP fitted with torch layers and with each few-bit configuration (tools/convergence_demo.py); the DCT estimator at lr 1.0', f'{D} 7.4'),
    ('r06_dct_rows_big.txt', 'the kernel pair and the torch.fft formulation at 2^17 and 2^18 rows (512-point tiles)', f'{D} 7.3'),
    ('r06_dct_rows_5x.txt', 'the kernel pair and the torch.fft formulation at 5 x 2^k rows (1280 .. 40960)', f'{D} 7.3'),
    ('r06_dct_rows_3x.txt', 'the kernel pair and the torch.fft formulation at 3 x 2^k rows (768 .. 49152)', f'{D} 7.3'),
    ('transform_rows_odd.txt', 'tools/transform_rows_bench.py: both kernel pairs at 7 x 2^k, 9 x 2^k and 15 x 2^k rows against the torch.fft formulation and against the next power of two', f'{E} 8.3'),
    ('transform_zext.txt', "tools/transform_zext_bench.py: the zero-extended kernel pairs at 12800 and 51200 rows against F.pad + the plain call, the plain call on N' real rows and the torch.fft formulation", f'{E} 8.6'),
    ('r06_dct_variants.txt', 'the sampled-DCT variants measured in round 6, phases compiled out, per-workgroup timeline', f'{D} 7.5'),
    ('r06_dct_sorted_samples.txt', 'the samples sorted by residue class once, in pass A, instead of tested by every pass-B workgroup: pass B 17.3 -> 12.7 us', f'{D} 5'),
    ('r06_dct_serve_lanes.txt', 'pass B writing a sampled row with 16 / 8 / 4 lanes: 4 shipped (pass B -8 %)', f'{D} 7.5'),
    ('r06_dct_rounds.txt', 'both DCT passes against the number of workgroups (features swept): a fixed 7-9 us plus 7.5 ns per workgroup', f'{D} 7.5'),
    ('r07_transform_columns.txt', 'both sampled-transform kernel pairs per feature column on structured inputs: kernel / fp32 reference error ratios (tests/test_gpu_transform_columns.py)', f'{D} 6'),
    ('crs_bench.json', 'tools/sketch_bench.py (CRS=1): LinearCRS forward extra and weight-gradient part on the kernels against the torch formulation; rocprofv3 kernel times, gather byte-floor fraction', f'{E} 8.2'),
    ('variance_bench.json', "tools/variance_bench.py: the variance estimator's postprocess on the kernels (row_moments + one GEMM + sum_squares) against the fp32 formulation it replaced and the float64 fallback; row_moments against two vector_norm calls, byte-floor fraction", f'{E} 8.9'),
    ('dropout_bench.json', "tools/dropout_bench.py: fewbit.functional.dropout / dropout_add forward + backward against torch's dropout at 16384 x 768 / 3072, bf16 and fp32; bytes saved for backward; the kernel alone against its byte floor", f'{E} 8.11'),
    ('quant_linear_bench.json', 'tools/quant_linear_bench.py: fewbit.QuantizedLinear at 2 / 4 / 8 bits forward + backward beside nn.Linear and RandomizedLinear(dct, 0.2) at 16384 x 768 / 3072, bf16 and fp32; bytes kept; weight-gradient error; pack / unpack alone against their byte floors', f'{E} 8.17'),
    ('layer_norm_bench.json', 'tools/layer_norm_bench.py: fewbit.QuantizedLayerNorm at 2 / 4 / 8 bits forward + backward beside nn.LayerNorm at 16384 x 768 / 3072, bf16 and fp32; bytes kept; gradient errors; the forward and backward entry points alone against their byte floors', f'{E} 8.18'),
    ('rms_norm_bench.json', 'tools/rms_norm_bench.py: fewbit.QuantizedRMSNorm at 2 / 4 / 8 bits forward + backward beside nn.RMSNorm at 16384 x 768 / 3072 / 4096, bf16 and fp32; bytes kept; gradient errors; the forward and backward entry points alone against their byte floors and against the layer-norm entry points', f'{E} 8.19'),
    ('add_norm_bench.json|add_norm_bench_run?.json', 'tools/add_norm_bench.py: fewbit.DropoutAddLayerNorm / DropoutAddRMSNorm at 2 / 4 / 8 bits forward + backward beside dropout_add + the quantized norm and beside torch at 16384 x 768 / 3072 (layer norm, p = 0.1) and 16384 x 4096 (RMS norm, prenorm), bf16 and fp32; bytes kept; the fused entry points alone against their byte floors (add_norm_bench.json and run2 .. run5: the five invocations whose minima are quoted)', f'{E} 8.21'),
    ('glu_bench.json', 'tools/glu_bench.py: fewbit.functional.glu_quantized at 2 / 4 / 8 bits forward + backward beside F.silu(gate) * up at 16384 x 3072 / 11008, bf16 and fp32; bytes kept; gradient errors; the forward and backward entry points alone against their byte floors', f'{E} 8.22'),
    ('gated_mlp_bench.json', 'tools/gated_mlp_bench.py: fewbit.QuantizedGatedMLP(fused=True) at 2 / 4 / 8 bits forward + backward beside fused=False and the torch MLP at 16384 x 4096 -> 11008 / 768 -> 3072, bf16 and fp32, five alternating invocations; bytes saved for backward; the glu_backward_product entry point alone against its byte floor', f'{E} 8.23'),
    ('roberta_add_norm_bf16.json', 'tools/roberta_bench.py --dtype bf16 --dropout fewbit --layer-norm fused and --layer-norm fewbit, one run each: RoBERTa-base b128 x s128 with the sublayer endings on DropoutAddLayerNorm against dropout + QuantizedLayerNorm', f'{E} 8.21'),
    ('roberta_layer_norm_bf16.json', 'tools/roberta_bench.py --dtype bf16 --layer-norm fewbit: RoBERTa-base b128 x s128 with every nn.LayerNorm swapped for QuantizedLayerNorm(bits=4), alone and with the GELU swap', f'{E} 8.18'),
    ('dropout_kernel_times.txt', 'rocprofv3 --kernel-trace over tools/dropout_bench.py: per-dispatch durations of the dropout kernel and of torch\'s forward / backward dropout kernels, per shape', f'{E} 8.11'),
    ('roberta_dropout_bf16.json', 'tools/roberta_bench.py --dtype bf16 --dropout fewbit: RoBERTa-base b128 x s128 with every nn.Dropout swapped, alone and with the GELU swap', f'{E} 8.11'),
    ('signed_transform_bench.json', 'tools/signed_transform_bench.py: the sampled DCT / DFT with the signs of the seed against the unsigned _zext_seeded calls at 16384 x 768 / 3072, p = 3276, bf16 and fp32: HIP events per call and rocprofv3 per pass', f'{E} 8.15'),
    ('signed_transform_kernel_stats.csv', 'rocprofv3 --kernel-trace --stats over tools/signed_transform_bench.py --trace: every kernel of the signed and unsigned calls', f'{E} 8.15'),
    ('roberta_signed_dct_*.json', 'tools/roberta_bench.py --table --matmul dct, use_sign_flips off and on: RoBERTa-base b128 x s128 step time and peak memory, bf16 and fp32', f'{E} 8.15'),
    ('convergence_demo_signed_*.txt', "tools/convergence_demo.py with the signed-DCT arm: bf16 at the usual step size and at SGD lr 1.0, where the unsigned DCT arm diverges", f'{D} 7.4'),
    ('transform_one_text_isa_identity.txt', 'tools/isa_digest.py --diff --rename: machine code of all 2143 device functions before / after pass A and pass B of the plain pairs became one kernel template each (798 kernels renamed, none changed)', f'{E} 8.16'),
    ('unit_fold_isa_identity.txt', "tools/isa_digest.py --diff: machine code of all 2888 device functions before / after the companion units' host code and element access moved into fewbit_unit.h (none changed)", f'{E} 8.27'),
    ('refusal_digest.txt', 'tools/refusal_digest.py: status and message of every refusal of the quant, glu, norm, fused-norm and dropout entry points, single faults and pairs (tests/test_refusals_host.py compares)', f'{E} 8.27'),
    ('core_fold_isa_identity.txt', "tools/isa_digest.py --diff: machine code of all 2888 device functions before / after the activation unit's dispatch, checks and launch code were said once (none changed)", f'{E} 8.28'),
    ('core_refusal_digest.txt', 'tools/core_refusal_digest.py: status and message of every refusal of the activation launches, describes, tune and codec entry points, single faults and pairs, plain and with FEWBIT_HIP_VALIDATE=1; recorded from the library before the fold (tests/test_core_refusals_host.py compares)', f'{E} 8.28'),
    ('core_fold_plan_digest.txt', 'tools/plan_digest.py --digest: lines and sha256 per entry point and tune setting of the 1 449 569 plans of the sweep on a 256-CU MI355X, the same from the parent and from the tree', f'{E} 8.28'),
    ('core_fold_speed.txt', 'the four activation entry points at 16384 x 768 and at n = 4096, bf16 and fp32, from the parent and from the tree with the folded host code, alternating five times', f'{E} 8.28'),
    ('cross_entropy_bench.json', 'tools/cross_entropy_bench.py: fewbit.functional.cross_entropy forward + backward, plain and with inplace_backward, beside F.cross_entropy on the logits as given, on their fp32 copy and under autocast at 16384 x 32000 / 50265 / 128256, bf16 and fp32; bytes saved for backward; peak allocation; the forward and backward entry points alone against their byte floors', f'{E} 8.29'),
    ('cross_entropy_isa_identity.txt', 'tools/isa_digest.py --diff: machine code of all 2888 device functions before / after fewbit_xent.hip was added (6 new)', f'{E} 8.29'),
    ('unit_fold_speed*.txt','the launch-bound entry-point arms of quant_linear_bench, dropout_bench, glu_bench and layer_norm_bench from the parent and from the tree with fewbit_unit.h, alternating five times', f'{E} 8.27'),
    ('signed_transform_isa_identity.txt', 'tools/isa_digest.py --diff: machine code of all 1915 device functions before / after the signed pass A was added (228 new)', f'{E} 8.15'),
    ('moments_isa_identity.txt', 'tools/isa_digest.py --diff: machine code of all 1890 device functions before / after fewbit_moments.hip was added (13 new)', f'{E} 8.9'),
    ('r06_dct_stagger.txt|r06_dct_fused_upper_bound.txt|r06_dct_inter16.txt', 'DCT experiments not kept: staggered starts, both passes in one launch (timing only), a bf16 intermediate', 'EXPERIMENTS.md'),
    ('r0?_roberta_table_*.json', "tools/roberta_bench.py --table: the reference README's RoBERTa table per dtype and estimator", f'{D} 7.4'),
    ('r0?_roberta_ab_fp32.txt|r0?_roberta_ab_bf16.txt|r0?_roberta_randomized_insitu*.json', 'the randomized RoBERTa step, arms interleaved in one process; its GPU time by kernel class', f'{D} 7.4'),
    ('r06_roberta_overlap_ab.txt', 'the estimators on a side stream beside the layer GEMMs: slower, not kept', f'{E} round 6'),
    ('r06_isa_identity.txt', 'tools/isa_digest.py: machine code of all 628 device functions before / after the round-6 source clean-up', f'{D} 9'),
    ('transform_zext_isa_identity.txt', 'tools/isa_digest.py --diff: machine code of all 1320 device functions before / after the zero-extended pairs were added (570 new)', f'{E} 8.6'),
    ('store_values_isa_identity.txt', "tools/isa_digest.py --diff: machine code of all 1890 device functions before / after pass B's vector store became one function of fewbit_fft4.h", f'{E} 8.8'),
    ('linear_routes_bit_identity.txt', 'sha256 of the output, the kept tensors and the gradients of every route of linear_grp / linear_crs: two runs of the parent and one of the tree with one call path, side by side', f'{E} 8.8'),
    ('tail_body_isa_identity.txt', "tools/isa_digest.py --diff and --where: the 168 fp16 activation kernels before / after the register barrier of Elem<FEWBIT_F16>::store -- 159 differ only behind their tile loop, 7 have the same loop with registers renumbered, 2 (threshold forward) a rescheduled address add", f'{E} 8.14'),
    # ---- experiments (kept as records; the design quotes only their conclusions)
    ('r02_launch_shape_sweep_*.txt|r03_*shape_sweep*.txt|r03_backward_size_crossover.txt', 'launch shape, groups per lane and size crossovers of the activation kernels', f'{D} 3.1'),
    ('r03_ablation_*.txt|r03_kernels_r02_vs_r03_ab.txt|r03_inplace_stores.txt|r04_inplace_*.txt', 'one stage compiled out at a time; in-place stores; round-to-round A/B', f'{D} 7.1; {E} 6'),
    ('r02_forward_head_variants.txt|r02_fp32_split_layout_ab.txt|r02_wave_timeline_trace.txt|r03_wave_priority_and_early_head.txt|r03_saddr_addressing_ab.txt|r04_state_staging_ab.txt',
     'forward head variants, fp32 split layout, wave timelines, s_setprio, saddr addressing, staged state stores', f'{E} 6'),
    ('r04_insitu_*.txt|r05_insitu_pmc*.txt', 'the forward right behind the GEMM that feeds it: time, launch shape, counters', f'{D} 7.2; {E} 5'),
    ('r0?_all_fp32_*.txt|r0?_all_patterns_more.txt|r0?_ragged_sweep.txt', 'exhaustive sweeps: all 2^32 fp32 patterns, every (gy, level) product, every remainder', f'{D} 6'),
    ('r04_injected_child_failure.txt', "a failing rank's traceback reaches the parent", f'{D} 8'),
    ('r04_sketch_balance.txt|r04_sketch_hostcost.txt|r04_sketch_preconvert.txt', 'slice balance, host cost and the conversion pass of the dense sketches', f'{D} 4'),
    ('r05_gen_bench*.txt|r0?_gaussian_ablation.txt|r05_sketch_*_ab.txt|r06_gen_bench.txt', 'generator cost beside an MFMA stream; A/B of the sketch data paths', f'{D} 4; {E} 3.1'),
    ('r05_roberta_ab_*.txt|r05_roberta_power_*.txt|r05_box_fingerprints.txt|r05_roberta_table_*_width_rule.json',
     'round 5: the width rule of fp32 input and the GPU-pool forensics behind it (closed; not to be repeated)', f'{D} 4, 9; {E} 5.1'),
    ('README.md', 'this index', ''),
]


def covered(name: str) -> bool:
    return any(fnmatch.fnmatch(name, pat) for row in ROWS for pat in row[0].split('|'))


def main() -> int:
    files = sorted(p.name for p in (ROOT / 'profiles').iterdir() if p.is_file())
    missing = [f for f in files if not covered(f)]
    if missing:
        sys.stderr.write('files under profiles/ without a row in tools/profiles_index.py: ' + ', '.join(missing) + '\n')
        return 1
    if len(sys.argv) > 1 and sys.argv[1] == '--check':
        return 0
    lines = ['Evidence kept per round (`rNN_*`; a round\'s core set is regenerated by `bash tools/profile_round.sh rNN` through `gpurun`). Generated by',
             '`python tools/profiles_index.py`, which fails when a file has no row. Where several rounds hold the same file the newest is the one quoted.', '',
             '| file(s) | what it is | quoted in |', '|---|---|---|']
    for pats, what, where in ROWS:
        n = sum(1 for f in files if any(fnmatch.fnmatch(f, p) for p in pats.split('|')))
        lines.append(f"| {', '.join('`' + p + '`' for p in pats.split('|'))} ({n}) | {what} | {where} |")
    (ROOT / 'profiles' / 'README.md').write_text('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
