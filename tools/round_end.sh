#!/bin/bash
# Round-end evidence on the GPU box: gpu tests, default bench line, kernel-trace summaries (default = three streams,
# and --serial-streams = every kernel un-contended, which the roofline object refers to), PMC traffic passes.
set -x
R=$GRAFT_REPO_ROOT
cd $R
OUT=${OUT:-$R/build/evidence}      # where every file of the evidence set is written
mkdir -p $OUT
python -m pytest tests -q -m gpu 2>&1 | tail -3 > $OUT/gpu_tests.txt
python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.txt 2>&1; echo "rc=$?" >> $OUT/smoke.txt
cd /tmp && export TMPDIR=/tmp
# PMC passes FIRST: the default bench line below then reports roofline.traffic from a table measured on these very sources
[ -n "$SKIP_PMC" ] || rocprofv3 --pmc FETCH_SIZE -d $OUT/prof_fetch -- python $R/bench.py --no-cpu-baseline --no-roofline --no-fidelity --steps 2 --warmup 1 > $OUT/prof_fetch.log 2>&1
[ -n "$SKIP_PMC" ] || rocprofv3 --pmc WRITE_SIZE -d $OUT/prof_write -- python $R/bench.py --no-cpu-baseline --no-roofline --no-fidelity --steps 2 --warmup 1 > $OUT/prof_write.log 2>&1
cd $R
[ -n "$SKIP_PMC" ] || python tools/pmc_dump.py $(find $OUT/prof_fetch -name "*.db" | head -1) "" > $OUT/pmc_fetch.txt 2>&1
[ -n "$SKIP_PMC" ] || python tools/pmc_dump.py $(find $OUT/prof_write -name "*.db" | head -1) "" > $OUT/pmc_write.txt 2>&1
# the table bench.py's roofline.traffic reads, stamped with the hash of the kernel sources (copy both into profiles/)
[ -n "$SKIP_PMC" ] || python tools/pmc_traffic.py $OUT/pmc_fetch.txt $OUT/pmc_write.txt --json $OUT/traffic_table.json > $OUT/pmc_traffic.txt 2>&1
[ -n "$SKIP_PMC" ] || cp $OUT/traffic_table.json profiles/traffic_table.json
# round 6: the same command beyond the old 2^24-pixel envelope -> profiles/best_batch.json (bench.py's config.best_batch)
for B in 256 320 384 512 768 1024; do
  python bench.py --batch $B --no-cpu-baseline --no-roofline > $OUT/bench_b$B.json 2> $OUT/bench_b$B.err
done
python tools/best_batch.py $OUT/bench_b256.json $OUT/bench_b320.json $OUT/bench_b384.json $OUT/bench_b512.json $OUT/bench_b768.json $OUT/bench_b1024.json > $OUT/best_batch.json && cp $OUT/best_batch.json profiles/best_batch.json
python bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err
python bench.py --no-cpu-baseline --no-roofline --no-fidelity --steps 10 --warmup 5 | python -c "import sys, json; r = json.loads([l for l in sys.stdin if l.startswith('{')][-1]); print('config.best_batch as the bench line reports it:', r['config']['best_batch'])" > $OUT/best_batch_check.txt 2>&1
cd /tmp
rocprofv3 --kernel-trace --stats -d $OUT/prof_kt -- python $R/bench.py --no-cpu-baseline --no-fidelity --no-roofline --steps 9 --warmup 3 > $OUT/prof_kt.log 2>&1
rocprofv3 --kernel-trace --stats -d $OUT/prof_ks -- python $R/bench.py --full --no-cpu-baseline --no-fidelity --serial-streams --steps 9 --warmup 3 > $OUT/prof_ks.log 2>&1
cd $R
python tools/rocpd_stats.py $(find $OUT/prof_kt -name "*.db" | head -1) 60 > $OUT/kernel_stats.txt
python tools/rocpd_stats.py $(find $OUT/prof_ks -name "*.db" | head -1) 60 > $OUT/kernel_stats_serial.txt
find $OUT -name "*.db" -delete
grep -h '^{' $OUT/prof_ks.log | tail -1 > $OUT/bench_serial.json
# BASELINE configs 4 and 5 (host-bound at these batch sizes): bench line with the roofline leg + kernel trace each
C4="--textual transdec_postnorm::L4_H1024_A16_F4096 --batch 128"
C5="--visual torchvision::resnet101 --textual transdec_postnorm::L1_H2048_A32_F8192 --batch 64"
# their own PMC tables (bytes per launch depend on the workload's shapes): roofline.traffic of these two lines
for C in 4 5; do
  [ -n "$SKIP_PMC" ] && break
  if [ $C = 4 ]; then CF="$C4"; else CF="$C5"; fi
  cd /tmp
  rocprofv3 --pmc FETCH_SIZE -d $OUT/prof_fetch$C -- python $R/bench.py --no-cpu-baseline --no-roofline --no-fidelity --steps 2 --warmup 1 $CF > $OUT/prof_fetch$C.log 2>&1
  rocprofv3 --pmc WRITE_SIZE -d $OUT/prof_write$C -- python $R/bench.py --no-cpu-baseline --no-roofline --no-fidelity --steps 2 --warmup 1 $CF > $OUT/prof_write$C.log 2>&1
  cd $R
  python tools/pmc_dump.py $(find $OUT/prof_fetch$C -name "*.db" | head -1) "" > $OUT/pmc_fetch_config$C.txt 2>&1
  python tools/pmc_dump.py $(find $OUT/prof_write$C -name "*.db" | head -1) "" > $OUT/pmc_write_config$C.txt 2>&1
  python tools/pmc_traffic.py $OUT/pmc_fetch_config$C.txt $OUT/pmc_write_config$C.txt --json $OUT/traffic_table_config$C.json > $OUT/pmc_traffic_config$C.txt 2>&1
  cp $OUT/traffic_table_config$C.json profiles/traffic_table_config$C.json
  rm -rf $OUT/prof_fetch$C $OUT/prof_write$C
done
# (round 6: WITH the fidelity leg -- the bf16 step against the fp32 step on the timed batch of these two configurations)
python bench.py --full --no-cpu-baseline $C4 > $OUT/bench_config4.json 2> $OUT/bench_config4.err
python bench.py --full --no-cpu-baseline $C5 > $OUT/bench_config5.json 2> $OUT/bench_config5.err
cd /tmp
rocprofv3 --kernel-trace --stats -d $OUT/prof_c4 -- python $R/bench.py --no-cpu-baseline --no-fidelity --no-roofline --serial-streams --steps 9 --warmup 3 $C4 > $OUT/prof_c4.log 2>&1
rocprofv3 --kernel-trace --stats -d $OUT/prof_c5 -- python $R/bench.py --no-cpu-baseline --no-fidelity --no-roofline --serial-streams --steps 9 --warmup 3 $C5 > $OUT/prof_c5.log 2>&1
cd $R
python tools/rocpd_stats.py $(find $OUT/prof_c4 -name "*.db" | head -1) 40 > $OUT/kernel_stats_serial_config4.txt
python tools/rocpd_stats.py $(find $OUT/prof_c5 -name "*.db" | head -1) 40 > $OUT/kernel_stats_serial_config5.txt
find $OUT -name "*.db" -delete; rm -rf $OUT/prof_c4 $OUT/prof_c5 $OUT/prof_kt $OUT/prof_ks $OUT/prof_fetch $OUT/prof_write
# round 5: the reference's module graph through stock PyTorch-ROCm (MIOpen / hipBLASLt) on this GPU, next to the product's step
[ -n "$SKIP_STOCK" ] || timeout 420 python bench.py --no-cpu-baseline --no-fidelity --no-roofline --stock-pytorch-baseline --steps 20 --warmup 10 > $OUT/bench_stock_pytorch_baseline.json 2> $OUT/bench_stock_pytorch_baseline.err
[ -n "$SKIP_STOCK" ] || timeout 420 python bench.py --no-cpu-baseline --no-fidelity --no-roofline --stock-pytorch-baseline --steps 20 --warmup 10 $C4 > $OUT/bench_stock_pytorch_baseline_config4.json 2> $OUT/bench_stock_pytorch_baseline_config4.err
[ -n "$SKIP_STOCK" ] || timeout 420 python bench.py --no-cpu-baseline --no-fidelity --no-roofline --stock-pytorch-baseline --steps 20 --warmup 10 $C5 > $OUT/bench_stock_pytorch_baseline_config5.json 2> $OUT/bench_stock_pytorch_baseline_config5.err
# round 5: the fused conv3 backward against the launches it replaces; JPEG decode throughput of the input pipeline
timeout 300 python tools/bench_conv3_bwd.py > $OUT/conv3_bwd.txt 2>&1
timeout 300 python tools/bench_jpeg.py > $OUT/bench_jpeg.txt 2>&1
cat $OUT/gpu_tests.txt
