/*
 * video_to_cu_depth -- native (C, no Python) form of the predictor step, same command line and
 * exit-status contract as the reference's driver:
 *
 *     video_to_cu_depth <yuv> <width> <height> <qp>          (cwd = HM's bin/ directory)
 *
 * replaces  system("python video_to_cu_depth.py <yuv> <w> <h> <qp>")
 * (/root/reference/HM-16.5_Test_AI/source/App/TAppEncoder/TAppEncCfg.cpp:2317-2321): reads
 * Thr_info.txt and model_2000000_qpXX~YY.dat.* from the cwd, writes cu_depth.dat, exits 0 on
 * success and 1 on any failure (HM asserts on the status).  It is also the smallest complete
 * consumer of include/ethcnn.h from plain C (built with gcc -std=c99 -pedantic), i.e. what an
 * in-process hook in HM would call.
 *
 * ETHCNN_SYNTHETIC_SEED=<n> [ETHCNN_HEAD_GAIN=<g>] opts into seeded synthetic weights when the
 * trained .data blob is absent (it is not in the reference repository); ETHCNN_DEVICE=<n> picks
 * the GPU; ETHCNN_DEVICES=0,1,2,... shards the frames over several GPUs from this ONE process
 * (ethcnn_predict_yuv_file_sharded: a worker thread per listed device, no collective; a device
 * may be listed twice).  ETHCNN_FC1_PLAN=2|3: the opted-in plan is checked against the restored
 * checkpoint (ethcnn_check_fc1_plan); a refusal is printed and the run continues with the exact
 * plan -- the encoder asserts a zero exit status.  ETHCNN_INPUT_BIT_DEPTH=8..16 and
 * ETHCNN_INPUT_CHROMA_FORMAT=400|420|422|444 name the source format of the file (HM's InputBitDepth
 * and InputChromaFormat; the command line is fixed); unset: 8-bit 4:2:0; a bad value is exit 1 with a
 * message.  ETHCNN_FC1_PLAN_AUDIT=<N> (read only when ETHCNN_FC1_PLAN is set and the guard accepted
 * the plan) audits the plan on min(N, frames) evenly spaced frames of this file before it is trusted
 * (ethcnn_audit_plan_yuv_file: plan against exact plan at the run's QP, Thr_info.txt as the candidate),
 * with the single-launch pass off so that the audited frames take the 16-bit path of the whole run),
 * prints one line with the numbers and continues with the exact plan when anything is over 1e-4 or
 * the audit itself fails; a
 * malformed value, a source that is not 8-bit 4:2:0 or more than one device is exit 1 before anything
 * runs.  ETHCNN_TIMING=1 prints where the command's
 * wall time goes (stderr): the blocking system() of the caller sees all of it.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

#include "ethcnn.h"

static int fail(const ethcnn_ctx* ctx, const char* what) {
    fprintf(stderr, "video_to_cu_depth: %s: %s\n", what, ethcnn_last_error(ctx));
    return 1;
}

static double now_ms(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec * 1e3 + (double)ts.tv_nsec * 1e-6;
}

static int file_exists(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) return 0;
    fclose(f);
    return 1;
}

/* an integer environment variable: 1 = unset (the default stays), 0 = taken, -1 = not an integer */
static int env_int(const char* name, int* value) {
    const char* text = getenv(name);
    char* end;
    long v;
    if (!text || !*text) return 1;
    v = strtol(text, &end, 10);
    if (*end != '\0' || v < -100000 || v > 100000) return -1;
    *value = (int)v;
    return 0;
}

/* Thr_info.txt in All-Intra token order (up1 down1 up2 down2 up3 down3) on the k / 1024 grid, the nearest k each; 0 when the file does
 * not hold six values inside the simulator's ranges (the audit then compares no search) */
static int read_thr_k(const char* path, ethcnn_sim_thr* thr) {
    FILE* f = fopen(path, "r");
    double v[6];
    int i, n = 0;
    if (!f) return 0;
    while (n < 6 && fscanf(f, "%lf", &v[n]) == 1) ++n;
    fclose(f);
    if (n < 6) return 0;
    for (i = 0; i < 6; ++i) {
        const double x = v[i] * 1024.0;
        int k;
        if (!(x >= -1.5 && x <= 1024.5)) return 0;
        k = (int)(x + 1.5) - 1; /* floor(x + 0.5) for x >= -1.5 */
        if (i & 1) thr->down_k[i >> 1] = k;
        else thr->up_k[i >> 1] = k;
    }
    for (i = 0; i < 3; ++i)
        if (thr->up_k[i] < 0 || thr->up_k[i] > 1024 || thr->down_k[i] < -1 || thr->down_k[i] > 1024) return 0;
    return 1;
}

/* the accepted plan against the exact plan on min(n_audit, frames) evenly spaced frames of the file itself; always 0: a failure of the
 * audit itself is printed and takes the fallback of a refusal */
static int audit_plan(ethcnn_ctx* ctx, const char* yuv, int width, int height, int qp, int n_audit) {
    const int plan = ethcnn_get_fc1_plan(ctx);
    const float tol = 1e-4f; /* the plans' contract */
    struct stat st;
    ethcnn_sim_thr thr;
    ethcnn_audit_result r;
    int64_t frames, count, step;
    uint64_t over, classes;
    int have_thr, rc;
    if (stat(yuv, &st) != 0 || width <= 0 || height <= 0) return 0; /* (the prediction reports a file it cannot read) */
    frames = (int64_t)st.st_size / ((int64_t)width * height * 3 / 2);
    count = n_audit < frames ? n_audit : frames;
    if (plan == 0 || count <= 0) return 0;
    step = frames / count;
    have_thr = read_thr_k("Thr_info.txt", &thr);
    /* with the single-launch pass off: a few frames would run as that pass, which computes exactly under every plan, while the run over
     * the whole file takes the 16-bit path; the audit must take the path it audits */
    (void)ethcnn_set_small_pass_launch(ctx, 0);
    rc = ethcnn_audit_plan_yuv_file(ctx, yuv, width, height, qp, plan, 0, step, count, tol, have_thr ? &thr : NULL, &r);
    (void)ethcnn_set_small_pass_launch(ctx, 1);
    if (rc != ETHCNN_OK) { /* an audit that cannot run (memory, a read error) is no reason to fail the encode: the exact plan is always right */
        fprintf(stderr, "video_to_cu_depth: plan %d audit failed: %s\nvideo_to_cu_depth: continuing with the exact plan (0)\n", plan, ethcnn_last_error(ctx));
        (void)ethcnn_set_fc1_plan(ctx, 0);
        return 0;
    }
    over = r.stats.over_tol[0] + r.stats.over_tol[1] + r.stats.over_tol[2];
    classes = r.stats.class_diff[0] + r.stats.class_diff[1] + r.stats.class_diff[2];
    fprintf(stderr, "video_to_cu_depth: plan %d audit over %lld frames (step %lld): max |dp| %.3g %.3g %.3g, values over %g: %llu, ", plan, (long long)count,
            (long long)step, (double)r.stats.max_abs[0], (double)r.stats.max_abs[1], (double)r.stats.max_abs[2], (double)tol, (unsigned long long)over);
    if (have_thr) fprintf(stderr, "classes that differ: %llu, CTUs whose search differs: %llu, ", (unsigned long long)classes, (unsigned long long)r.stats.search_diff_ctus);
    else fprintf(stderr, "classes that differ: n/a, CTUs whose search differs: n/a, ");
    fprintf(stderr, "fast passes %d/%d: %s\n", (int)r.fast_passes, (int)r.passes,
            r.fast_passes == 0 ? "these frames run as single-launch passes, which compute exactly under every plan: nothing to audit, plan kept"
                               : over ? "continuing with the exact plan (0)" : "plan kept");
    if (over && r.fast_passes) (void)ethcnn_set_fc1_plan(ctx, 0);
    return 0;
}

int main(int argc, char** argv) {
    ethcnn_ctx* ctx = NULL;
    ethcnn_options opt;
    char model[64], data[96];
    int64_t nframes = 0;
    ethcnn_source_format fmt = {8, 420};
    int width, height, qp, rc, ndev = 0, devices[64], n_audit = 0;
    const char* plan_env = getenv("ETHCNN_FC1_PLAN");
    const char* seed = getenv("ETHCNN_SYNTHETIC_SEED");
    const char* dev = getenv("ETHCNN_DEVICE");
    const char* devs = getenv("ETHCNN_DEVICES");
    const char* timing = getenv("ETHCNN_TIMING");
    const double t0 = now_ms();
    double t_create, t_weights, t_guard, t_predict = t0, runtime_ms = 0.0, create_ms = 0.0;

    if (argc != 5) {
        fprintf(stderr, "usage: %s <yuv> <width> <height> <qp>\n", argv[0]);
        return 1;
    }
    width = atoi(argv[2]);
    height = atoi(argv[3]);
    qp = atoi(argv[4]);
    if (env_int("ETHCNN_INPUT_BIT_DEPTH", &fmt.bit_depth) < 0 || env_int("ETHCNN_INPUT_CHROMA_FORMAT", &fmt.chroma_format) < 0 ||
        fmt.bit_depth < 8 || fmt.bit_depth > 16 ||
        (fmt.chroma_format != 400 && fmt.chroma_format != 420 && fmt.chroma_format != 422 && fmt.chroma_format != 444)) {
        fprintf(stderr, "video_to_cu_depth: bad ETHCNN_INPUT_BIT_DEPTH (8..16) or ETHCNN_INPUT_CHROMA_FORMAT (400, 420, 422, 444)\n");
        return 1;
    }
    if (devs && *devs) { /* "0,1,2,3": worker k on the k-th entry */
        const char* q = devs;
        while (*q && ndev < 64) {
            char* end;
            const long d = strtol(q, &end, 10);
            if (end == q || d < 0) { fprintf(stderr, "video_to_cu_depth: bad ETHCNN_DEVICES '%s'\n", devs); return 1; }
            devices[ndev++] = (int)d;
            q = (*end == ',') ? end + 1 : end;
            if (*end != ',' && *end != '\0') { fprintf(stderr, "video_to_cu_depth: bad ETHCNN_DEVICES '%s'\n", devs); return 1; }
        }
    }
    if (ndev == 0) devices[ndev++] = dev ? atoi(dev) : 0;
    if (plan_env && *plan_env) { /* ETHCNN_FC1_PLAN_AUDIT is read only beside an opted-in plan */
        /* one to six decimal digits and nothing else (no sign, no blank): the Python launcher's rule */
        const char* text = getenv("ETHCNN_FC1_PLAN_AUDIT");
        if (text && *text && strspn(text, "0123456789") == strlen(text) && strlen(text) <= 6) n_audit = atoi(text);
        else if (text && *text) {
            fprintf(stderr, "video_to_cu_depth: bad ETHCNN_FC1_PLAN_AUDIT (a number of frames of one to six digits, 0 = no audit)\n");
            return 1;
        }
        if (n_audit > 0 && (fmt.bit_depth != 8 || fmt.chroma_format != 420 || ndev > 1)) {
            fprintf(stderr, "video_to_cu_depth: ETHCNN_FC1_PLAN_AUDIT reads 8-bit 4:2:0 files on one GPU only (anything else is not built)\n");
            return 1;
        }
    }
    memset(&opt, 0, sizeof opt);
    opt.device = devices[0];
    if (ethcnn_create(&ctx, &opt) != ETHCNN_OK) return fail(NULL, "create");
    t_create = now_ms();
    if (ethcnn_set_source_format(ctx, &fmt) != ETHCNN_OK) { rc = fail(ctx, "source format"); goto out; }
    if (ethcnn_load_thresholds(ctx, "Thr_info.txt") != ETHCNN_OK) { rc = fail(ctx, "Thr_info.txt"); goto out; }
    if (ethcnn_model_name_for_qp(qp, model, sizeof model) != ETHCNN_OK) { rc = fail(ctx, "model name"); goto out; }
    snprintf(data, sizeof data, "%s.data-00000-of-00001", model);
    if (file_exists(data) || !seed) {
        if (ethcnn_load_checkpoint(ctx, model) != ETHCNN_OK) { rc = fail(ctx, model); goto out; }
    } else {
        const char* gain = getenv("ETHCNN_HEAD_GAIN");
        if (ethcnn_load_synthetic(ctx, (uint64_t)strtoull(seed, NULL, 10), gain ? atof(gain) : 1.0) != ETHCNN_OK) {
            rc = fail(ctx, "synthetic weights");
            goto out;
        }
    }
    t_weights = now_ms();
    if (ethcnn_get_fc1_plan(ctx) != 0) {
        const int g = ethcnn_check_fc1_plan(ctx, ethcnn_get_fc1_plan(ctx), NULL, NULL);
        if (g == ETHCNN_ERR_PLAN_REFUSED) {
            fprintf(stderr, "video_to_cu_depth: %s\nvideo_to_cu_depth: continuing with the exact plan (0)\n", ethcnn_last_error(ctx));
            (void)ethcnn_set_fc1_plan(ctx, 0);
        } else if (g != ETHCNN_OK) { rc = fail(ctx, "plan check"); goto out; }
        else if (n_audit > 0 && audit_plan(ctx, argv[1], width, height, qp, n_audit) != 0) { rc = 1; goto out; }
    }
    t_guard = now_ms();
    if (ethcnn_predict_yuv_file_sharded(ctx, devices, ndev, argv[1], width, height, qp, "cu_depth.dat", &nframes) != ETHCNN_OK) {
        rc = fail(ctx, argv[1]);
        goto out;
    }
    t_predict = now_ms();
    printf("%lld frames predicted -> cu_depth.dat\n", (long long)nframes);
    if (timing && atoi(timing) != 0) {
        (void)ethcnn_get_startup_times(ctx, &runtime_ms, &create_ms);
        if (getenv("ETHCNN_T0_MS")) fprintf(stderr, "video_to_cu_depth timing: spawn -> main %.1f ms\n", t0 - atof(getenv("ETHCNN_T0_MS")));
        fprintf(stderr, "video_to_cu_depth timing (ms since main): create %.1f (HIP runtime init %.1f, context %.1f) | thresholds + weights %.1f | plan guard %.1f | "
                        "predict (%d worker%s) %.1f | total in main %.1f\n",
                t_create - t0, runtime_ms, create_ms - runtime_ms, t_weights - t_create, t_guard - t_weights, ndev, ndev == 1 ? "" : "s",
                t_predict - t_guard, t_predict - t0);
    }
    rc = 0;
    {   /* cu_depth.dat is complete and renamed into place: nothing is left that an orderly teardown would save.  ethcnn_destroy (12-40 ms)
         * and the HIP runtime's exit handlers (~45 ms) are a quarter of this command's wall time on the reference's own 768x512 case, and
         * the caller blocks on it (TAppEncCfg.cpp:2317-2321); the driver reclaims the process's GPU resources either way.
         * ETHCNN_FAST_EXIT=0 keeps the orderly path (sanitizer / leak-check runs). */
        const char* fe = getenv("ETHCNN_FAST_EXIT");
        if (!(fe && atoi(fe) == 0)) {
            fflush(stdout);
            fflush(stderr);
            _exit(0);
        }
    }
out:
    ethcnn_destroy(ctx);
    if (timing && atoi(timing) != 0) fprintf(stderr, "video_to_cu_depth timing: destroy %.1f ms\n", now_ms() - t_predict);
    return rc;
}
