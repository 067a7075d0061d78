// sage2_amd/csrc/sage2ov_cli.cpp -- `sage2ov`: the SAGE2 command line (main.cpp:384-521): -f | -l, -k, -o, -p, -i, -m, -M, -s, -d, -h.
// -M 3 (the default) writes <outdir>/<prefix>.reads and <prefix>.graph3, which the unchanged reference continues from (SAGE2 ... -i P -m 4, main.cpp:141-148);
// -m 1..4 with -M 5 | 6 | 7 is the whole assembly in one process on the graph that stays resident: step 5 with the library's solver, step 6 (extendContigs,
// <prefix>_contig.fasta) and step 7 (makeScaffolds, <prefix>_scaffold.fasta).
// --flowNetwork writes <outdir>/input.cs2 (step 5's flow network, with the genome-size estimate) and --flowSolution FILE applies a solver's output.cs2 and writes
// <prefix>.graph5: after step 4, or with -m 5 from <inputPrefix>.reads and <inputPrefix>.graph4.  No outside solver is started here; --flowSolve is the whole of step 5 with
// the library's own solver on the device (with -s it leaves input.cs2 and its output.cs2 too).
// --contigs [--genomeSize G] also writes <prefix>_contig.fasta, printGraph's file (main.cpp:246), for the graph after step 4 or a P.graph4 / 5 / 6 (-m 5 | 6 | 7).
#include <getopt.h>
#include <sys/stat.h>
#include <unistd.h>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <memory>
#include <vector>
#include "sage2ov.hpp"
#include "sage2ov_multi.h"

using namespace std;
using namespace sage2ov;

static void printUsage() {
    cout << "USAGE:\n\tsage2ov [options] -f <inputFile> -k <minOverlap>   (steps 1-3 of SAGE2 on an MI355X)\n"
            "\tsage2ov [options] -l <listInput> -k <minOverlap>\n\n";
}
static void printListOfArgs() {
    cout << "\t-f|--fileInput <string>\tinterleaved FASTA/FASTQ(.gz)\n\t-l|--listInput <string>\tlist file (f1=/f2=/f=)\n"
            "\t-k|--minOverlap <int>\tminimum overlap (required)\n\t-o|--outputDir <string>\n\t-p|--prefix <string>\t[untitled]\n"
            "\t-i|--inputPrefix <string>\t[prefix]\n\t-m|--minStep <int>\t[1]\n\t-M|--maxStep <int>\t[3] (4 = simplified graph P.graph4; 5 = copy counts, P.graph5; 6 = extended contigs, P_contig.fasta and P.graph6;\n"
            "\t\t\t7 = scaffolds, P_scaffold.fasta: with -m 1..4 the whole run in one process, the graph stays on the device; steps 6-7 need -f or -l)\n"
            "\t-s|--saveAll\n\t-d|--debug\n\t-g|--gpu <int>\tHIP device ordinal [0]\n"
            "\t-G|--gpus <int>\tsteps 2-3 on this many GPUs of the node (devices gpu .. gpu+G-1): reads and index replicated, probe pass\n"
            "\t\t\trange-partitioned, records / flags / edge and survivor buckets exchanged with RCCL over xGMI [1]\n"
            "\t--contigs\t\talso write <prefix>_contig.fasta (printGraph): after step 4, or with -m 5|6|7 from <inputPrefix>.reads and <inputPrefix>.graph4|5|6\n"
            "\t--genomeSize <int>\tgenome size for the N50 / N90 of --contigs [0; with --flowNetwork or --flowSolution: the estimate]\n"
            "\t--flowNetwork\t\tstep 5 up to its solver: estimate the genome size and write <outputDir>input.cs2 (after step 4, or with -m 5 from <inputPrefix>.graph4)\n"
            "\t--flowSolution <string>\tstep 5 after its solver: apply this output.cs2 to the flows and write <prefix>.graph5\n"
            "\t--flowSolve\t\tthe whole of step 5 with the solver on the device: write <prefix>.graph5 (with -s also <outputDir>input.cs2 and output.cs2)\n"
            "\t--extend\t\twith -m 6: load <inputPrefix>.graph5, map the mate pairs of -f|-l, estimate the insert sizes, merge contigs by mate-pair\n"
            "\t\t\tsupport until a round merges nothing (the first loop of extendContigs; --paths and --shortOverlaps add the others) and write <prefix>.graph6 [--genomeSize: the estimate on the loaded graph]\n"
            "\t--paths\t\t\twith -m 6 --extend: after the first loop, the loops of findPathSupports and findPathSupportsNew (merges by path support)\n"
            "\t--shortOverlaps\t\twith -m 6 --extend: after those, the loop of mergeShortOverlaps (joins of contigs whose mates give a summed gap of at most 0);\n"
            "\t\t\t--extend --paths --shortOverlaps is the whole extendContigs\n"
            "\t--scaffold\t\twith -m 7: load <inputPrefix>.graph6, map the mate pairs of -f|-l, estimate the insert sizes, join contigs that share no node by\n"
            "\t\t\tmate-pair links (the five loops of makeScaffolds) and write <prefix>_scaffold.fasta; with -m 6 --extend: go on from the merged graph, no new estimate\n\t-h|--help\n\n";
}
static string trimBack(string s, const string& pat) { size_t e = s.find_last_not_of(pat); return e == string::npos ? "" : s.substr(0, e + 1); }
static double now() { return chrono::duration<double>(chrono::steady_clock::now().time_since_epoch()).count(); }

int main(int argc, char* argv[]) {
    const double tMain = now(); const bool timing = getenv("SAGE2OV_TIMING") != nullptr;
    int minStep = 1, maxStep = 3, gpu = 0, gpus = 1, failRank = -1; bool shareGpu = false, forceMulti = false; unsigned minOverlap = 0; bool contigs = false, extend = false, paths = false, shortOverlaps = false, scaffold = false, flowNetwork = false, flowSolve = false, genomeSizeGiven = false, maxGiven = false; string flowSolution; unsigned long long genomeSize = 0; bool saveAll = false, debugging = false, fFlag = false, lFlag = false;
    string fileInput, listInput, outputDir, prefixName = "untitled", inputPrefix;
    static struct option opts[] = {{"help", no_argument, 0, 'h'}, {"fileInput", required_argument, 0, 'f'}, {"minOverlap", required_argument, 0, 'k'},
        {"listInput", required_argument, 0, 'l'}, {"outputDir", required_argument, 0, 'o'}, {"prefix", required_argument, 0, 'p'},
        {"inputPrefix", required_argument, 0, 'i'}, {"minStep", required_argument, 0, 'm'}, {"maxStep", required_argument, 0, 'M'},
        {"saveAll", no_argument, 0, 's'}, {"debug", no_argument, 0, 'd'}, {"gpu", required_argument, 0, 'g'}, {"gpus", required_argument, 0, 'G'},
        {"share-gpu", no_argument, 0, 1001},      // rehearsal: all ranks on device `gpu`, exchanges by device copies instead of RCCL (a box with fewer GPUs than ranks)
        {"fail-rank", required_argument, 0, 1003},  // tests: this rank of a multi-GPU run fails before its first step (the run must end non-zero, not hang)
        {"contigs", no_argument, 0, 1004}, {"genomeSize", required_argument, 0, 1005}, {"flowNetwork", no_argument, 0, 1006}, {"flowSolution", required_argument, 0, 1007}, {"extend", no_argument, 0, 1008}, {"scaffold", no_argument, 0, 1009}, {"paths", no_argument, 0, 1010}, {"shortOverlaps", no_argument, 0, 1011}, {"flowSolve", no_argument, 0, 1012},
        {"force-multi", no_argument, 0, 1002},    // the multi-GPU code path (RCCL communicator, the four exchanges) even with one GPU
        {0, 0, 0, 0}};
    int c, oi = 0;
    while ((c = getopt_long(argc, argv, "hf:l:k:o:p:i:m:M:sdg:G:", opts, &oi)) != -1) {
        switch (c) {
            case 'h': cout << "\n"; printUsage(); printListOfArgs(); exit(0);
            case 'f': fileInput = optarg; fFlag = true; break;
            case 'l': listInput = optarg; lFlag = true; break;
            case 'k': minOverlap = atoi(optarg); break;
            case 'o': outputDir = optarg; if (outputDir != "") outputDir = trimBack(outputDir, "/") + "/"; break;   // main.cpp:438-442
            case 'p': prefixName = optarg; break;
            case 'i': inputPrefix = optarg; break;
            case 'm': minStep = atoi(optarg); if (minStep < 1) minStep = 1; break;
            case 'M': maxStep = atoi(optarg); if (maxStep > 7) maxStep = 7; maxGiven = true; break;
            case 's': saveAll = true; break;
            case 'd': debugging = true; break;
            case 'g': gpu = atoi(optarg); break;
            case 'G': gpus = atoi(optarg); if (gpus < 1) gpus = 1; break;
            case 1001: shareGpu = true; break;
            case 1002: forceMulti = true; break;
            case 1003: failRank = atoi(optarg); break;
            case 1004: contigs = true; break;
            case 1005: genomeSize = strtoull(optarg, nullptr, 10); genomeSizeGiven = true; break;
            case 1006: flowNetwork = true; break;
            case 1007: flowSolution = optarg; break;
            case 1012: flowSolve = true; break;
            case 1008: extend = true; break;
            case 1010: paths = true; break;
            case 1011: shortOverlaps = true; break;
            case 1009: scaffold = true; break;
            case '?': cout << "\n"; exit(0);
            default: cout << "[ERROR] Wrong command line arguments!\n\n"; exit(0);
        }
    }
    if (fFlag && lFlag) { cout << "[ERROR] Options -f|--fileInput and -l|--listInput are mutually exclusive!\n\n"; exit(0); }
    if (flowSolve && flowSolution != "") { cout << "[ERROR] Options --flowSolve and --flowSolution are mutually exclusive!\n\n"; exit(0); }
    // the whole run: -m 1..4 through -M 5 | 6 | 7 on one context.  A run that crosses step 5 solves the flow itself (an outside solver cannot run in the middle)
    const bool through5 = minStep <= 4 && maxStep >= 6, ends5 = minStep <= 4 && maxStep == 5 && !flowNetwork && flowSolution == "";
    if (through5 && (flowNetwork || flowSolution != "")) { cout << "[ERROR] -M " << maxStep << " runs step 5 with the solver on the device: --flowNetwork and --flowSolution stop at step 5 (-M 5), an outside solver cannot run in the middle.\n"; exit(0); }
    if (through5 || ends5) flowSolve = true;
    const bool step5 = flowNetwork || flowSolve || flowSolution != "";
    if (step5 && !maxGiven && maxStep < minStep) maxStep = minStep;                          // (`-m 5 --flowSolution FILE` needs no -M)
    bool allSet = true;                                                                     // main.cpp:498-521
    if (fileInput == "" && listInput == "" && minStep <= 1) { cout << "[ERROR] One of the options -f|--fileInput or -l|--listInput is required.\n"; allSet = false; }
    if (minOverlap == 0) { cout << "[ERROR] Option -k|--minOverlap is required.\n"; allSet = false; }
    if ((extend || scaffold) && !maxGiven && maxStep < minStep) maxStep = minStep;           // (`-m 6 --extend` and `-m 7 --scaffold` need no -M)
    if (maxStep < minStep) { cout << "[ERROR] maxStep should not be smaller than minStep!\n\n"; allSet = false; }
    if (inputPrefix == "") inputPrefix = prefixName;
    if (!allSet) { cout << "\n"; printUsage(); cout << "(For more information run sage2ov -h)\n\n"; exit(0); }
    if (step5 && maxStep < 4) { cout << "[ERROR] --flowNetwork and --flowSolution need the graph after step 4: run with -M 4 (or -m 5 on the files of such a run).\n"; exit(0); }
    if (minStep > 5 && step5) { cout << "[ERROR] --flowNetwork and --flowSolution work on the graph after step 4 (-m 5 at the most).\n"; exit(0); }
    if (through5 && fileInput == "" && listInput == "") { cout << "[ERROR] -M " << maxStep << " maps the mate pairs in step 6 and needs the mate pairs (-f or -l).\n"; exit(0); }
    if (extend && (minStep != 6 || (fileInput == "" && listInput == ""))) { cout << "[ERROR] --extend works on <inputPrefix>.graph5 (-m 6) and needs the mate pairs (-f or -l).\n"; exit(0); }
    if (paths && !(extend && minStep == 6)) { cout << "[ERROR] --paths goes with -m 6 --extend.\n"; exit(0); }
    if (shortOverlaps && !(extend && minStep == 6)) { cout << "[ERROR] --shortOverlaps goes with -m 6 --extend.\n"; exit(0); }
    if (scaffold && (!(minStep == 7 || (minStep == 6 && extend)) || (fileInput == "" && listInput == ""))) { cout << "[ERROR] --scaffold works on <inputPrefix>.graph6 (-m 7), or after --extend (-m 6), and needs the mate pairs (-f or -l).\n"; exit(0); }
    if (minStep > 4 && !contigs && !step5 && !extend && !scaffold) { cout << "[ERROR] A run that starts at step " << minStep << " says what it does: --flowSolve | --flowNetwork | --flowSolution (-m 5), --extend (-m 6), --scaffold (-m 7) or --contigs; the whole run is -m 1..4 with -M 5 | 6 | 7.\n"; exit(0); }
    (void)debugging;
    if (outputDir != "") { string cmd = "mkdir -p " + outputDir; if (system(cmd.c_str())) {} }     // utils.cpp:45
    ofstream logStream((outputDir + prefixName + ".log").c_str());
    logStream << "***********************************************************************************************************\n"
              << "\tEXECUTING PROGRAM: sage2ov (MI355X-native SAGE2), " << sage2ov_version() << "\n"
              << (listInput != "" ? "\t  INPUT LIST PATH: " + listInput : "\t  INPUT FILE PATH: " + fileInput) << "\n"
              << "\t OUTPUT DIRECTORY: " << outputDir << "\n\t    OUTPUT PREFIX: " << prefixName << "\n\t  MINIMUM OVERLAP: " << minOverlap << "\n"
              << "\t       START STEP: " << minStep << "\n\t         END STEP: " << maxStep << "\n\t   SAVE ALL FILES: " << (saveAll ? "TRUE" : "FALSE") << "\n"
              << "***********************************************************************************************************\n\n";
    const int lastStep = maxStep > 4 ? 4 : maxStep;
    try {
        const bool multi = (gpus > 1 || forceMulti) && lastStep >= 3 && minStep <= 3;
        // (the device opens in the background while step 1 reads its files)
        Context ctx((uint16_t)minOverlap, lastStep == 1 ? SAGE2OV_DEVICE_NONE : gpu, 0, 0, multi ? (unsigned)gpus : 1u, minStep <= 1 ? SAGE2OV_FLAG_ASYNC_DEVICE : 0u);
        ReadLoader loaderObj(ctx);
        double t0 = now();
        if (timing) fprintf(stderr, "[cli] start-up (context, device) %8.1f ms\n", 1e3 * (t0 - tMain));
        // the whole run from step 1: the mate table of step 6 comes from step 1's own pass (-f: library 1; -l: the list's own numbering)
        const bool pairFromReads = minStep <= 1 && through5;
        if (pairFromReads) ctx.check(sage2ov_reads_pair_library(ctx.get(), 1));
        if (minStep <= 1) {                                                                  // main.cpp:37-61
            logStream << "STEP 1: organizing reads\n";
            if (listInput != "") loaderObj.loadFromList(listInput); else loaderObj.readDatasetInBytes(fileInput);
            loaderObj.organizeReads();
            auto s = loaderObj.stats();
            logStream << "\tTotal reads: " << s.total_reads << "\n\tGood reads: " << s.good_reads << "\n\tNumber of unique reads: " << s.unique_reads
                      << "\n\tAverage read length: " << s.average_read_length << "\n\tStep 1 in " << now() - t0 << " sec.\n";
            if (lastStep == 1 || saveAll) { double tw = now(); loaderObj.saveReadsInFile(outputDir + prefixName + ".reads"); logStream << "\t" << prefixName << ".reads written in " << now() - tw << " sec.\n"; }
        } else {
            loaderObj.loadReadsFromFile(outputDir + inputPrefix + ".reads");                 // main.cpp:70-74 / :101-104
            logStream << "\tNumber of unique reads: " << loaderObj.numberOfUniqueReads << " (loaded)\n";
        }
        auto writeContigs = [&](OverlapGraph& graphObj) {                                     // main.cpp:246: printGraph(outputDir + prefix + "_contig", 0)
            double tw = now();
            auto cs = graphObj.printGraph(outputDir + prefixName + "_contig", false, genomeSize);
            logStream << "\t" << prefixName << "_contig.fasta written in " << now() - tw << " sec.\n\t  Number of Contigs: " << cs.contigs << " (" << cs.written << " in the file)\n\t     Longest Contig: " << cs.longest
                      << "\n\t     Genome Covered: " << cs.covered << " BP\n\t                N50: " << cs.n50 << " BP (" << cs.n50_ordinal << ")\n\t                N90: " << cs.n90 << " BP (" << cs.n90_ordinal << ")\n";
        };
        auto copyCounts = [&]() {                                                             // main.cpp:199-203, without the solver
            if (!step5) return;
            double t5 = now();
            uint64_t est = 0; ctx.check(sage2ov_genome_size_estimate(ctx.get(), &est));
            sage2ov_copycount_stats cs{}; ctx.check(sage2ov_copycount_stats_get(ctx.get(), &cs));
            logStream << "STEP 5: copy counts\n";
            for (uint32_t i = 0; i < cs.rounds; i++) {                                        // copycountEstimator.cpp:41, :47
                const bool fin = cs.agreed && i + 1 == cs.rounds;
                string line = "\tGenome Size: " + to_string(cs.estimate[i]) + (fin ? " (Final estimation)" : " (Estimation " + to_string(i + 1) + ")") + "\n";
                logStream << line; if (flowNetwork) cout << line;
            }
            if (flowNetwork) {
                ctx.check(sage2ov_flow_network_save(ctx.get(), (outputDir + "input.cs2").c_str()));
                ctx.check(sage2ov_copycount_stats_get(ctx.get(), &cs));
                logStream << "\t          Number of nodes: " << cs.nodes << "\n\t          Number of edges: " << cs.edges << "\n\t             Simple edges: " << cs.simple
                          << "\n\t  Edges used exactly once: " << cs.once << "\n\tEdges used more than once: " << cs.many << "\n\tinput.cs2 written: " << cs.network_nodes << " nodes, "
                          << cs.network_arcs << " arcs\n";
            }
            if (flowSolution != "") {
                ctx.check(sage2ov_flow_solution_load(ctx.get(), flowSolution.c_str()));
                ctx.check(sage2ov_copycount_stats_get(ctx.get(), &cs));
                logStream << "\t         Flow from T to S: " << cs.t_to_s_flow << "\n\t  Flow different in edges: " << cs.flow_different << "\n";
                ctx.check(sage2ov_graph5_save(ctx.get(), (outputDir + prefixName + ".graph5").c_str()));
                logStream << "\t" << prefixName << ".graph5 written\n";
            }
            if (flowSolve) {                                                                  // main.cpp:199-203 with main_cs2 (copycountEstimator.cpp:359) on the device
                ctx.check(sage2ov_flow_network_build(ctx.get()));
                if (saveAll) ctx.check(sage2ov_flow_network_save(ctx.get(), (outputDir + "input.cs2").c_str()));
                sage2ov_mcf_stats ms{}; ctx.check(sage2ov_flow_solve(ctx.get(), 0, &ms));
                if (saveAll) ctx.check(sage2ov_flow_solution_save(ctx.get(), (outputDir + "output.cs2").c_str()));
                ctx.check(sage2ov_flow_solution_commit(ctx.get()));
                ctx.check(sage2ov_copycount_stats_get(ctx.get(), &cs));
                logStream << "\tMin-cost flow: " << ms.nodes << " nodes, " << ms.arcs << " arcs, cost " << ms.total_cost << "; " << ms.phases << " phases, " << ms.rounds << " rounds, "
                          << ms.pushes << " pushes, " << ms.relabels << " relabels, " << ms.price_updates << " price updates, " << 64 * ms.price_words << "-bit prices, in "<< (ms.build_ms + ms.solve_ms) / 1000.0 << " sec.\n"
                          << "\t         Flow from T to S: " << cs.t_to_s_flow << "\n\t  Flow different in edges: " << cs.flow_different << "\n";
                if (!through5 || saveAll) {                                                   // (a run that goes on writes it with -s only, as the reference does)
                    ctx.check(sage2ov_graph5_save(ctx.get(), (outputDir + prefixName + ".graph5").c_str()));
                    logStream << "\t" << prefixName << ".graph5 written\n";
                }
            }
            if (!genomeSizeGiven) genomeSize = est;
            logStream << "\tStep 5 (" << (flowSolve ? "with" : "without") << " its solver) in " << now() - t5 << " sec.\n";
        };
        // the mate pairs of -f | -l and the insert sizes (main.cpp:236-240, :265-270).  fromReads: the table comes from step 1's own pass (the context staged the input with
        // pairing on: neither a second pass over the file nor a search of the read store); else the input is read again, as the restart routes do
        auto mapMates = [&](bool fromReads) {
            double tm = now();
            if (fromReads) ctx.check(sage2ov_mates_from_reads(ctx.get()));
            else if (listInput != "") ctx.check(sage2ov_mates_add_list(ctx.get(), listInput.c_str()));
            else ctx.check(sage2ov_mates_add_file(ctx.get(), fileInput.c_str(), nullptr, 1));
            if (timing) fprintf(stderr, "[cli] mate table (%s) %8.1f ms\n", fromReads ? "from step 1's pass" : "second pass over the input", 1e3 * (now() - tm));
            ctx.check(sage2ov_mates_estimate(ctx.get()));
        };
        auto step6 = [&](bool fromReads, bool doPaths, bool doShort, bool saveGraph6) {        // main.cpp:236-244, extendContigs (mergeContigs.cpp:37-113): its first loop, the others by doPaths and doShort
            double t6 = now();
            logStream << "STEP 6: map mate pairs & merge by mate-pair support\n";
            mapMates(fromReads);
            logStream << "\nIn function mergeContigs().\n";
            uint64_t rounds = 0, merged = 0;
            const int rc = sage2ov_extend_by_supports(ctx.get(), genomeSizeGiven ? genomeSize : 0, &rounds, &merged);
            sage2ov_extend_stats xs{}; ctx.check(sage2ov_extend_stats_get(ctx.get(), &xs));
            logStream << "\tRounds of findMatepairSupports: " << rounds << " (" << xs.total.entries << " supported pairs listed, " << xs.total.refused << " refused, " << xs.total.blocked
                      << " blocked, " << xs.total.pairs_deleted << " edges deleted, " << xs.total.entries_copied << " list entries written)\n";
            ctx.check(rc);
            if (doPaths) {                                                                  // the second and third loop (mergeContigs.cpp:62-99)
                static const char* const name[2] = {"findPathSupports", "findPathSupportsNew"};
                for (int variant = 0; variant < 2; variant++) {
                    uint64_t r = 0, m = 0;
                    const int rc2 = sage2ov_extend_by_paths(ctx.get(), genomeSizeGiven ? genomeSize : 0, variant, &r, &m);
                    logStream << "\tRounds of " << name[variant] << ": " << r << " (" << m << " merges)\n";
                    ctx.check(rc2); merged += m;
                }
            }
            if (doShort) {                                                          // the fourth loop (mergeContigs.cpp:101-110)
                uint64_t r = 0, m = 0;
                const int rc2 = sage2ov_extend_by_short_overlaps(ctx.get(), genomeSizeGiven ? genomeSize : 0, &r, &m);
                sage2ov_scaffold_stats ss{}; ctx.check(sage2ov_extend_short_stats_get(ctx.get(), &ss));
                logStream << "\tRounds of mergeShortOverlaps: " << r << " (" << ss.total.rows << " rows, " << ss.total.below_threshold << " below the threshold, " << ss.total.skipped << " skipped, "
                          << ss.total.blocked << " blocked; lists joined by overlap " << ss.total.overlaps << ", concatenated " << ss.total.concatenated
                          << ", with a gap " << ss.total.gapped << "; " << m << " merges)\n";
                ctx.check(rc2); merged += m;
            }
            logStream << "\nTotal number of extended contigs: " << merged << "\n";
            if (saveGraph6) { ctx.check(sage2ov_graph6_save(ctx.get(), (outputDir + prefixName + ".graph6").c_str())); logStream << "\t" << prefixName << ".graph6 written\n"; }
            logStream << "\t" << (doPaths && doShort ? "Step 6" : doPaths ? "Loops 1-3 of step 6" : doShort ? "Loops 1 and 4 of step 6" : "First loop of step 6") << " in " << now() - t6 << " sec.\n";
        };
        auto step7 = [&](OverlapGraph& graphObj, bool mapFirst) {                             // main.cpp:263-290, makeScaffolds (scaffolding.cpp:31-98)
            double t7 = now();
            logStream << "STEP 7: merge contigs to get scaffolds\n";
            if (mapFirst) mapMates(false);                                                // (after step 6 its mates and its estimate stand, main.cpp:270)
            logStream << "\nIn function makeScaffolds().\n";
            uint64_t rounds = 0, merged = 0;
            const int rc = sage2ov_scaffold(ctx.get(), genomeSizeGiven ? genomeSize : 0, &rounds, &merged);
            sage2ov_scaffold_stats ss{}; ctx.check(sage2ov_scaffold_stats_get(ctx.get(), &ss));
            logStream << "\tRounds of mergeFinal: " << rounds << " (" << ss.total.rows << " rows, " << ss.total.below_threshold << " below the threshold, " << ss.total.skipped << " skipped, "
                      << ss.total.blocked << " blocked, " << ss.total.cycles << " cycles; lists joined by overlap " << ss.total.overlaps << ", concatenated " << ss.total.concatenated
                      << ", with a gap " << ss.total.gapped << ")\n";
            ctx.check(rc);
            logStream << "\nTotal number of merged scaffolds: " << merged << "\n";
            double tw = now();
            auto cs = graphObj.printGraph(outputDir + prefixName + "_scaffold", true, genomeSize);
            logStream << "\t" << prefixName << "_scaffold.fasta written in " << now() - tw << " sec.\n\t  Number of Scaffolds: " << cs.contigs << " (" << cs.written << " in the file)\n\tStep 7 in " << now() - t7 << " sec.\n";
        };
        auto step4 = [&](OverlapGraph& graphObj) {                                            // main.cpp:134-181
            double t4 = now();
            auto ss = graphObj.simplify();
            logStream << "STEP 4: simplify overlap graph\n\t   Nodes removed: " << ss.nodes_contracted << "\n\tDead ends and bubbles removed: " << ss.removed
                      << "\n\tLoop iterations: " << ss.loop_iterations << "\n\tEdges left: " << ss.edges << " carrying " << ss.reads_on_edges << " reads\n\tStep 4 in " << now() - t4
                      << " sec (device " << ss.device_ms / 1000.0 << ").\n";
            { double tw = now(); graphObj.saveSimplifiedGraphInFile(outputDir + prefixName + ".graph4"); logStream << "\t" << prefixName << ".graph4 written in " << now() - tw << " sec.\n"; }   // the file step 5 loads (main.cpp:196)
            copyCounts();
            if (contigs && maxStep < 6) writeContigs(graphObj);
            if (maxStep >= 6) { step6(pairFromReads, true, true, maxStep == 6 || saveAll); writeContigs(graphObj); }      // (main.cpp:246: printGraph after step 6)
            if (maxStep >= 7) step7(graphObj, false);
        };
        if (minStep > 4) {                                                                    // --contigs on the graph an earlier run or the reference left: P.graph4 / 5 / 6
            OverlapGraph graphObj(&loaderObj);
            graphObj.loadCompositeGraphFromFile(outputDir + inputPrefix + ".graph" + to_string(minStep - 1));
            copyCounts();
            if (extend) step6(false, paths, shortOverlaps, true);
            if (contigs) writeContigs(graphObj);
            if (scaffold) step7(graphObj, !extend);
        } else if (minStep == 4) {                                                            // main.cpp:141-148
            OverlapGraph graphObj(&loaderObj);
            graphObj.loadOverlapGraphFromFile(outputDir + inputPrefix + ".graph3");
            step4(graphObj);
        } else if (multi) {
            // steps 2-3 on `gpus` GPUs (sage2ov_multi.cpp): rank 0 = this context; the others import the organised read store
            t0 = now();
            vector<unique_ptr<Context>> others; vector<sage2ov_ctx*> all{ctx.get()}; vector<int> devs{gpu};
            {
                auto s = loaderObj.stats();
                vector<uint64_t> words((s.unique_reads + 1) * (uint64_t)s.words_per_read); vector<uint16_t> freq(s.unique_reads + 1);
                ctx.check(sage2ov_reads_export_words(ctx.get(), words.data(), words.size(), freq.data()));
                for (int r = 1; r < gpus; r++) {
                    const int dev = shareGpu ? gpu : gpu + r;
                    others.emplace_back(new Context((uint16_t)minOverlap, dev, 0, (unsigned)r, (unsigned)gpus));
                    others.back()->check(sage2ov_reads_import_words(others.back()->get(), words.data(), s.unique_reads, s.words_per_read, s.max_read_length, freq.data(), s.good_reads, s.total_bp));
                    all.push_back(others.back()->get()); devs.push_back(dev);
                }
            }
            string merr; int mrc = sage2ov_multi::run_steps23(all, devs, shareGpu, merr, failRank);
            if (mrc) throw Error(mrc, merr);
            sage2ov_index_stats is{}; ctx.check(sage2ov_index_stats_get(ctx.get(), &is)); sage2ov_overlap_stats os{}; ctx.check(sage2ov_overlap_stats_get(ctx.get(), &os));
            logStream << "STEPS 2-3 on " << gpus << (shareGpu ? " ranks sharing GPU " : " GPUs starting at ") << gpu << (shareGpu ? " (rehearsal transport)" : " (RCCL)") << "\n\t         Hash string length: " << is.hash_string_length
                      << "\n\t            Hash table size: " << is.slots << "\n\t Number of hash elements over threshold: " << is.long_buckets
                      << "\n     Total contained by extension: " << os.contained_extension << "\n          Total contained by size: " << os.contained_size
                      << "\n            Total left to explore: " << os.left_to_explore << "\n              Verified overlaps: " << os.verified_overlaps
                      << "\n     Total edges inserted: " << os.edges_inserted << "\n  Transitive edge removed: " << os.transitive_removed << "\n     Edges in the graph: " << os.edges
                      << "\n\tSteps 2-3 in " << now() - t0 << " sec.\n";
            OverlapGraph graphObj(&loaderObj);
            if (minStep == 1 && !saveAll) { double tw = now(); loaderObj.saveReadsInFile(outputDir + prefixName + ".reads"); logStream << "\t" << prefixName << ".reads written in " << now() - tw << " sec.\n"; }
            if (saveAll) { HashTable hashObj(&loaderObj); hashObj.saveHashTableInFile(outputDir + prefixName + ".hashTable"); }
            if (lastStep == 3 || saveAll) { double tw = now(); graphObj.saveOverlapGraphInFile(outputDir + prefixName + ".graph3"); logStream << "\t" << prefixName << ".graph3 written in " << now() - tw << " sec.\n"; }
            if (lastStep >= 4) step4(graphObj);
        } else if (lastStep >= 2) {
            HashTable hashObj(&loaderObj);
            t0 = now(); hashObj.hashPrefixesAndSuffix();                                      // main.cpp:76-77 (always rebuilt: P.hashTable is not read)
            auto is = hashObj.stats();
            logStream << "STEP 2: building hash table\n\t         Hash string length: " << is.hash_string_length << "\n\t            Hash table size: " << is.slots
                      << "\n\t Number of hash elements over threshold: " << is.long_buckets << "\n\tStep 2 in " << now() - t0 << " sec.\n";
            if (lastStep == 2) {
                if (minStep == 1 && !saveAll) { double tw = now(); loaderObj.saveReadsInFile(outputDir + prefixName + ".reads"); logStream << "\t" << prefixName << ".reads written in " << now() - tw << " sec.\n"; }
            }
            if (lastStep == 2 || saveAll) {                                                   // main.cpp:80-81: P.hashTable with -s or when the run ends here
                double tw = now(); hashObj.saveHashTableInFile(outputDir + prefixName + ".hashTable"); logStream << "\t" << prefixName << ".hashTable written in " << now() - tw << " sec.\n";
            }
            if (lastStep >= 3) {                                                              // main.cpp:92-132
                EconomyGraph economyObj(&hashObj);
                t0 = now(); economyObj.buildInitialOverlapGraph();
                auto os = economyObj.stats();
                logStream << "STEP 3: building overlap graph\n     Total contained by extension: " << os.contained_extension << "\n          Total contained by size: " << os.contained_size
                          << "\n            Total left to explore: " << os.left_to_explore << "\n              Verified overlaps: " << os.verified_overlaps << "\n";
                economyObj.buildOverlapGraphEconomy();
                os = economyObj.stats();
                logStream << "     Total edges inserted: " << os.edges_inserted << "\n  Transitive edge removed: " << os.transitive_removed << "\n";
                economyObj.sortEconomyGraph();
                OverlapGraph graphObj(&economyObj, &loaderObj);
                graphObj.convertGraph();
                logStream << "     Edges in the graph: " << economyObj.stats().edges << "\n\tStep 3 in " << now() - t0 << " sec.\n";
                if (minStep == 1 && !saveAll) { double tw = now(); loaderObj.saveReadsInFile(outputDir + prefixName + ".reads"); logStream << "\t" << prefixName << ".reads written in " << now() - tw << " sec.\n"; }
                if (lastStep == 3 || saveAll) { double tw = now(); graphObj.saveOverlapGraphInFile(outputDir + prefixName + ".graph3"); logStream << "\t" << prefixName << ".graph3 written in " << now() - tw << " sec.\n"; }      // main.cpp:120-131
                if (lastStep >= 4) step4(graphObj);
            }
        }
        if (timing) fprintf(stderr, "[cli] until the last file is written %8.1f ms\n", 1e3 * (now() - tMain));
        // every file is written and closed: leave without tearing down gigabytes of host vectors and the HIP runtime one allocation at a time
        // (0.25 s on a 10 M-read run; the kernel reclaims host and device memory of an exiting process at once)
        logStream.flush(); logStream.close(); cout.flush(); fflush(nullptr);
        if (!getenv("SAGE2OV_FULL_TEARDOWN")) _exit(0);
    } catch (const Error& e) {
        logStream << "sage2ov error " << e.code << " : " << e.what() << "!\n";               // utils.cpp:36-40 printError
        cerr << "sage2ov error " << e.code << ": " << e.what() << "\n";
        return EXIT_FAILURE;
    }
    return 0;
}
