# round 5 evidence on the final tree: the GPU suite; bench lines c2 (tiled, all-unique), c3,
# c4, c5 and rocprofv3 --kernel-trace --stats of each; FETCH_SIZE / WRITE_SIZE passes (one
# counter per pass) with the loads-only calibration; the SQ instruction mix of the lean
# kernel's stage-A ablations (c2, c3); smoke
R=$GRAFT_REPO_ROOT; cd $R && O=gpurun_out/${OUT:-r05final} && mkdir -p $O && export TMPDIR=/tmp
if [ -z "$NOTEST" ]; then
timeout -k 10 600 python -u -m pytest tests -m gpu -v --timeout 150 --timeout-method thread > $O/pytest_gpu.log 2>&1; rc=$?
tail -3 $O/pytest_gpu.log; grep -E "FAILED|ERROR" $O/pytest_gpu.log | head -20 || true
[ $rc -le 1 ] || { echo "pytest rc=$rc"; exit 1; }
fi
for spec in ${SPECS:-c2 c2u c3 c4 c5}; do
  wl=${spec%u}; extra=""; [ "$spec" != "$wl" ] && extra="--unique 1048576"
  timeout -k 10 500 python -u bench.py --full --workload $wl $extra > $O/bench_$spec.log 2>&1 || { echo "bench $spec failed"; tail -20 $O/bench_$spec.log; exit 1; }
  (cd /tmp && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $R/$O/prof_$spec -o $spec -- python3 $R/bench.py --no-cpu --no-pcie --no-serve --workload $wl $extra --steps 5 > $R/$O/prof_$spec.log 2>&1) || { echo "rocprof $spec failed"; exit 1; }
done
if [ -z "$NOPMC" ]; then
for wl in c2 c3 c4 c5; do
  for c in FETCH_SIZE WRITE_SIZE; do
    (cd /tmp && timeout -s KILL 200 rocprofv3 --kernel-trace --pmc $c --output-format csv -d $R/$O/pmc_${c}_$wl -o run -- python3 $R/bench.py --no-cpu --no-pcie --no-serve --workload $wl --steps 2 --warmup 1 > $R/$O/pmc_${c}_$wl.log 2>&1) || { echo "pmc $c $wl failed"; exit 1; }
  done
done
(cd /tmp && timeout -s KILL 200 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $R/$O/pmc_cal -o run -- python3 $R/scripts/prof_modes.py --workload c2 --modes 15 --reps 2 > $R/$O/pmc_cal.log 2>&1) || { echo "pmc cal failed"; exit 1; }
for wl in c2 c3; do
  (cd /tmp && timeout -s KILL 240 rocprofv3 --kernel-trace --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_INSTS_VMEM_RD SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS --output-format csv -d $R/$O/sq_$wl -o run -- python3 $R/scripts/prof_modes.py --workload $wl --modes 0,15,16,17,18 --reps 2 > $R/$O/sq_$wl.log 2>&1) || { echo "sq $wl failed"; exit 1; }
  timeout -k 10 200 python -u scripts/prof_modes.py --workload $wl --modes 0,15,16,17,18,0 --reps 5 > $O/time_$wl.log 2>&1 || { echo "time $wl failed"; exit 1; }
done
fi
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1 && echo smoke ok || echo smoke failed
grep -h '"metric"' $O/bench_*.log | python3 -c "
import sys, json
for l in sys.stdin:
    d = json.loads(l); c = d['config']; print(c.get('workload'), c.get('unique_templates'), round(d['ms_per_step'],3), round(d['roofline']['kernel_ms'],3), round(d['roofline']['frac'],4), d.get('parity'), d.get('exact_path_requests'), d.get('undecided'))"
echo done
