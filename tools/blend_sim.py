# Wave-steps of the blend on the bench's 1 M scene and camera, from the oracle's lists (CPU only).
#   python3 tools/blend_sim.py                      the block shapes and batch sizes, threshold slack 0.1
#   python3 tools/blend_sim.py --slack 0.0          the same with another constant in the block threshold pmin - slack
#   python3 tools/blend_sim.py --staging-table      only the G = 8 staging table: slack 0.1 / 0.01 / 0.0, each with and without
#                                                   the blocks that are finished at a batch start left off that batch's lists
#   --drop-finished                                 adds that drop to the G = 8 rows of the default run
#   python3 tools/blend_sim.py --pixel-pass         only: how pixel-exact the G = 8 lists are (the kernel's block test, slack 0) —
#                                                   entries with no pixel that passes 0 <= -power <= L, passing pixels per entry,
#                                                   and the wave-steps of lists rebuilt from "some pixel passes"
#   python3 tools/blend_sim.py --wave-split         only: wave-steps if the two waves of a tile split its sixteen 4x4 blocks
#                                                   otherwise than by pixel rows (the eight longest lists to one wave)
#   python3 tools/blend_sim.py --skip-rate          only: the G = 8 wave-steps in which no pixel of the wave passes — what the any-lane
#                                                   branch of the trip loop skips — bucketed by the wave's live pixels at the batch
#                                                   start (the oracle's `stopped` flags on the range cut there): the table behind
#                                                   BLEND_FREE_MIN_LIVE (csrc/gs_render_kernels.h, NOTES.md Part XVII)
#   --n <Gaussians>                                 another size of the bench scene (--skip-rate --n 10000000: a deep scene)
#   --min-live <k>                                  the rule --skip-rate prices (default: BLEND_FREE_MIN_LIVE, read from the kernel header)
import argparse, os, sys, numpy as np
_root=os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_root, os.path.join(_root,'tools'), os.path.join(_root,'tests')): sys.path.insert(0,_p)
import synth, helpers
_ap=argparse.ArgumentParser()
_ap.add_argument('--slack',type=float,default=0.1)
_ap.add_argument('--drop-finished',action='store_true')
_ap.add_argument('--staging-table',action='store_true')
_ap.add_argument('--pixel-pass',action='store_true')
_ap.add_argument('--wave-split',action='store_true')
_ap.add_argument('--skip-rate',action='store_true')
_ap.add_argument('--n',type=int,default=1_000_000)
_ap.add_argument('--min-live',type=int,default=None)
ARGS=_ap.parse_args()
from oracle import binding as ob
N=ARGS.n; sh,cov=3,0
g=synth.scene(N); pods=ob.pack(sh,cov,g)
cam=helpers.default_camera(ob,1920,1080)
gt,mt=ob.gaussian_transform(sh_deg=0),ob.model_transform()
proj,tiles=ob.preprocess(sh,cov,pods,gt,mt,cam)
keys,idx=ob.build_keys(proj,tiles,120)
keys,idx=ob.sort_pairs(keys,idx)
tile=(keys>>np.uint64(32)).astype(np.int64)
D=len(keys); print('D',D)
p=proj[idx]
tx=(tile%120); ty=(tile//120)
mx=p['mx'].astype(np.float64); my=p['my'].astype(np.float64)
ca=p['ca'].astype(np.float64); cb=p['cb'].astype(np.float64); cc=p['cc'].astype(np.float64)
op=p['opacity'].astype(np.float64)
pmin=np.maximum(-np.log(255*op)-1e-3,-5.6)
def pmax(q2,q1,q0,lo,hi):
    t=np.clip(-0.5*q1/q2,lo,hi); return (q2*t+q1)*t+q0
def touches(rx0,rx1,ry0,ry1,slack=None,pmin=pmin):
    slack=ARGS.slack if slack is None else slack
    dxl=mx-rx1; dxh=mx-rx0; dyl=my-ry1; dyh=my-ry0
    inx=(dxl<=0)&(dxh>=0); iny=(dyl<=0)&(dyh>=0)
    m0=pmax(cc,cb*dxl,ca*dxl*dxl,dyl,dyh); m1=pmax(cc,cb*dxh,ca*dxh*dxh,dyl,dyh)
    m2=pmax(ca,cb*dyl,cc*dyl*dyl,dxl,dxh); m3=pmax(ca,cb*dyh,cc*dyh*dyh,dxl,dxh)
    m=np.maximum(np.maximum(m0,m1),np.maximum(m2,m3))
    return (inx&iny)|~(m<pmin-slack)
x0=tx*16+0.5; y0=ty*16+0.5
# position within tile list -> batch
start=np.searchsorted(tile,np.arange(8160)); pos=np.arange(D)-start[tile]; batch=pos//128
# --- the G = 8 staging: 4x4 blocks, 128-splat batches; a block all of whose 16 pixels have stopped (T < 1e-4, or outside the image) when a
# batch starts takes no entry in that batch.  The flags are the oracle's: blend(..., stopped=True) on every range cut at a multiple of 128.
_fin={}
def finished_at(mb):
    if mb not in _fin:
        nt=120*68
        rng=np.asarray(ob.tile_ranges(keys,nt)).reshape(nt,2).astype(np.int64)
        r=rng.copy(); r[:,1]=r[:,0]+np.minimum(rng[:,1]-rng[:,0],128*mb)
        _,st=ob.blend(proj,idx,np.ascontiguousarray(r.astype(np.uint32)),cam,stopped=True)
        pad=np.ones((68*16,1920),dtype=bool); pad[:1080]=st[:1080,:1920]>0      # rows outside the image count as finished
        _fin[mb]=pad.reshape(68*4,4,480,4).all(axis=(1,3))
    return _fin[mb]
def staging_g8(slack,drop):
    gb=tile*100000+batch
    u,inv=np.unique(gb,return_inverse=True)
    tot=0; s=0
    for hy in range(2):
        ls=[]
        for by in range(2):
            for bx in range(4):
                m=touches(x0+4*bx,x0+4*bx+3,y0+8*hy+4*by,y0+8*hy+4*by+3,slack)
                if drop:
                    br=ty*4+hy*2+by; bc=tx*4+bx
                    dead=np.zeros(D,dtype=bool)
                    for mb in range(1,int(batch.max())+1):
                        sel=batch==mb
                        dead[sel]=finished_at(mb)[br[sel],bc[sel]]
                    m=m&~dead
                tot+=m.sum(); ls.append(np.bincount(inv,weights=m,minlength=len(u)))
        s+=np.maximum.reduce(ls).sum()
    return int(tot),int(s)
if ARGS.staging_table:
    print('| block threshold slack | finished blocks | block entries | wave-steps |')
    for slack in (0.1,0.01,0.0):
        for drop in (False,True):
            e,s=staging_g8(slack,drop)
            print('| %g | %s | %d | %d |'%(slack,'left off' if drop else 'staged',e,s),flush=True)
    sys.exit(0)
if ARGS.skip_rate:
    # The G = 8 lists as the kernel builds them (slack 0, as under --pixel-pass).  A wave-step is step s of a wave (tile half) in a
    # batch, s below the longest of the wave's eight lists; a pixel passes it if it is live at the batch start and
    # 0 <= -power <= L for entry s of its block's list.  (Pixels that finish inside the batch count as live to its end, as the
    # flags are the batch start's: the skip share of the late steps of a batch is a little higher than printed.)
    pmin0=np.maximum(-np.log(255*op),-5.6)
    u,inv=np.unique(tile*1000+batch,return_inverse=True); nb=len(u)
    nbat=int(batch.max())+1
    live_px=np.zeros((nbat,68*16,1920),dtype=bool)        # [batch][y][x]: live at the batch start
    nt=120*68
    rng=np.asarray(ob.tile_ranges(keys,nt)).reshape(nt,2).astype(np.int64)
    for mb in range(nbat):
        if mb==0: live_px[0,:1080]=True
        else:
            r=rng.copy(); r[:,1]=r[:,0]+np.minimum(rng[:,1]-rng[:,0],128*mb)
            _,st=ob.blend(proj,idx,np.ascontiguousarray(r.astype(np.uint32)),cam,stopped=True)
            live_px[mb,:1080]=st[:1080,:1920]==0
    L=np.zeros((nb,16),dtype=np.int64)
    passed=np.zeros(nb*2*128,dtype=bool)                  # [(batch group, wave, step)]: some pixel of the wave passes
    txi=tx.astype(np.int64); tyi=ty.astype(np.int64)
    for r in range(4):
        for c in range(4):
            t=touches(x0+4*c,x0+4*c+3,y0+4*r,y0+4*r+3,0.0,pmin0)
            L[:,r*4+c]=np.bincount(inv,weights=t,minlength=nb)
            cs=np.cumsum(t); first=np.searchsorted(inv,np.arange(nb))         # (pairs are sorted by tile and position)
            rank=cs-1-(cs[first]-t[first])[inv]                                # position of an entry in its list
            any_px=np.zeros(D,dtype=bool)
            for j in range(4):
                for i in range(4):
                    dx=mx-(x0+4*c+i); dy=my-(y0+4*r+j)
                    pw=ca*dx*dx+cb*dx*dy+cc*dy*dy
                    any_px|=(pw<=0)&(pw>=pmin0)&live_px[batch,tyi*16+4*r+j,txi*16+4*c+i]
            sel=t&any_px
            passed[(inv[sel]*2+r//2)*128+rank[sel]]=True
    steps=np.stack([L[:,:8].max(1),L[:,8:].max(1)],axis=1).reshape(-1)          # [(batch group, wave)]
    blended=passed.reshape(nb*2,128).sum(1)
    gt_,gb_=u//1000,u%1000
    lv=np.zeros((nb,2),dtype=np.int64)
    for w in range(2):
        for j in range(8):
            rows=live_px[gb_,(gt_//120)*16+8*w+j]                               # [nb][1920]
            cols=(gt_%120)[:,None]*16+np.arange(16)[None,:]
            lv[:,w]+=np.take_along_axis(rows,cols,axis=1).sum(1)
    lv=lv.reshape(-1)
    run=lv>0                                                                    # a wave with no live pixel enters no loop
    print('batches',nb,'waves that enter the loop',int(run.sum()),'wave-steps (exact)',int(steps[run].sum()),
          'rounded up to even',int((((steps+1)//2)*2)[run].sum()))
    print('| live pixels at the batch start | wave-batches | wave-steps | no pixel passes | share |')
    for lo in range(1,129,8):
        b=run&(lv>=lo)&(lv<lo+8)
        ws,sk=int(steps[b].sum()),int((steps-blended)[b].sum())
        print('| %d..%d | %d | %d | %d | %s |'%(lo,lo+7,int(b.sum()),ws,sk,'%.4f'%(sk/ws) if ws else '-'))
    k=ARGS.min_live
    if k is None:
        import re
        k=int(re.search(r'constexpr uint32_t BLEND_FREE_MIN_LIVE = (\d+);',open(os.path.join(_root,'wgpu-3dgs-core_amd','csrc','gs_render_kernels.h')).read()).group(1))
    f=run&(lv>=k)
    ws,sk,odd=int(steps[f].sum()),int((steps-blended)[f].sum()),int((steps[f]&1).sum())
    print('rule: branch-free from %d live pixels: %d wave-batches of %d, %d wave-steps of them %d with no pixel passing (%.4f), %d odd step counts'
          %(k,int(f.sum()),int(run.sum()),ws,sk,sk/max(ws,1),odd))
    # the branch-free steps are those of the trips of four; the 0..3 left are branchy steps as before
    inloop=np.arange(128)[None,:]<(steps//4*4)[:,None]
    lb=int((passed.reshape(nb*2,128)&inloop)[f].sum()); ls=int((steps//4*4)[f].sum())-lb
    # against the loop that is branchy throughout (35 per blended step, 12 per skipped one, the count rounded up to even): a step of
    # a branch-free trip costs 34; the 0..3 remainder steps are branchy steps and cost what they did; an odd count saves its null step
    print('predicted change of SQ_INSTS_VALU per frame: of these wave-steps %d are in trips of four: -1 x %d blended, +22 x %d skipped; '
          '%d remainder steps unchanged; -12 x %d rounding steps: sum %d'
          %(lb+ls,lb,ls,ws-lb-ls,odd,-lb+22*ls-12*odd))
    sys.exit(0)
if ARGS.pixel_pass or ARGS.wave_split:
    # the G = 8 lists as the kernel builds them since NOTES.md Part XIV: threshold -L(k) = -ln(255 opacity), no constant, slack 0;
    # per (tile, batch) the lengths of the sixteen block lists (row-major; lists 0..7 are wave 0's), steps rounded up to even
    pmin0=np.maximum(-np.log(255*op),-5.6)
    u,inv=np.unique(tile*1000+batch,return_inverse=True); nb=len(u)
    L=np.zeros((nb,16),dtype=np.int64); Lx=np.zeros((nb,16),dtype=np.int64)
    ent=zero=pixpass=full=0
    for r in range(4):
        for c in range(4):
            t=touches(x0+4*c,x0+4*c+3,y0+4*r,y0+4*r+3,0.0,pmin0)
            L[:,r*4+c]=np.bincount(inv,weights=t,minlength=nb)
            if ARGS.pixel_pass:
                cnt=np.zeros(D,dtype=np.int64)
                for j in range(4):
                    for i in range(4):
                        dx=mx-(x0+4*c+i); dy=my-(y0+4*r+j)
                        pw=ca*dx*dx+cb*dx*dy+cc*dy*dy
                        cnt+=((pw<=0)&(pw>=pmin0))
                ent+=int(t.sum()); zero+=int((t&(cnt==0)).sum()); pixpass+=int(cnt[t].sum()); full+=int((t&(cnt==16)).sum())
                Lx[:,r*4+c]=np.bincount(inv,weights=(cnt>0),minlength=nb)
    ev=lambda x: ((x+1)//2)*2
    built=int(ev(L[:,:8].max(1)).sum()+ev(L[:,8:].max(1)).sum())
    print('batches',nb,'block entries',int(L.sum()),'wave-steps as built',built)
    if ARGS.pixel_pass:
        print('entries with no passing pixel %d (%.3f %%); passing pixels per entry %.2f of 16; entries whose 16 pixels all pass %d'
              %(zero,100.0*zero/ent,pixpass/ent,full))
        e=int(ev(Lx[:,:8].max(1)).sum()+ev(Lx[:,8:].max(1)).sum())
        print('wave-steps with lists rebuilt from "some pixel passes" %d (%.4f of as built)'%(e,e/built))
    if ARGS.wave_split:
        tl=u//1000
        first=np.searchsorted(tl,np.arange(8160))
        tile_tot=np.zeros((8160,16)); np.add.at(tile_tot,tl,L)
        for name,score in (('the eight longest lists of the first batch to one wave',None),
                           ('the eight longest by the whole tile\'s totals (not known when the tile starts)',tile_tot)):
            tot=0
            for t in range(8160):
                a=first[t]; b=first[t+1] if t+1<8160 else nb
                if a>=nb or tl[a]!=t: continue
                o=np.argsort(-(L[a] if score is None else score[t]),kind='stable')
                Lt=L[a:b]
                tot+=ev(Lt[:,o[:8]].max(1)).sum()+ev(Lt[:,o[8:]].max(1)).sum()
            print('%s: wave-steps %d (%.4f of as built)'%(name,int(tot),tot/built))
        srt=-np.sort(-L,axis=1)
        tot=int(ev(srt[:,0]).sum()+ev(srt[:,8]).sum())
        print('re-sorted in every batch (a bound: a lane\'s pixels are fixed): wave-steps %d (%.4f of as built)'%(tot,tot/built))
    sys.exit(0)
gid=tile*1000+batch   # (tile,batch) group id
def grp_sum(mask):
    u,inv=np.unique(gid,return_inverse=True); return np.bincount(inv,weights=mask,minlength=len(u))
# halves (current)
h=[touches(x0,x0+15,y0+8*k,y0+8*k+7) for k in range(2)]
cur=sum(grp_sum(m).sum() for m in h)
print('current wave-iterations (halves):',cur, 'per pair',cur/D)
# quadrants: wave w has quadrants (left,right) of half w
q={}
for qy in range(2):
    for qx in range(2):
        q[(qy,qx)]=touches(x0+8*qx,x0+8*qx+7,y0+8*qy,y0+8*qy+7)
new=0
for qy in range(2):
    a=grp_sum(q[(qy,0)]); b=grp_sum(q[(qy,1)]); new+=np.maximum(a,b).sum()
print('quadrant half-waves (max of 2 lists):',new,'ratio',new/cur, ' ideal sum/2:',sum(grp_sum(m).sum() for m in q.values())/2/cur)
# 8x4 blocks, quarter waves: wave w covers half w: 4 blocks: (bx in 0,1) x (by in 0,1) of size 8x4
e={}
new8=0
for hy in range(2):
    lists=[]
    for by in range(2):
        for bx in range(2):
            m=touches(x0+8*bx,x0+8*bx+7,y0+8*hy+4*by,y0+8*hy+4*by+3)
            lists.append(grp_sum(m))
    new8+=np.maximum.reduce(lists).sum()
    e[hy]=sum(l.sum() for l in lists)/4
print('8x4 quarter-waves (max of 4 lists):',new8,'ratio',new8/cur,' ideal:',sum(e.values())/cur)
# 4x4 blocks, eighth-waves (8 lanes x 2 px): wave w covers half w: 8 blocks (4 across x 2 down)
new16=0; ideal16=0
for hy in range(2):
    lists=[]
    for by in range(2):
        for bx in range(4):
            m=touches(x0+4*bx,x0+4*bx+3,y0+8*hy+4*by,y0+8*hy+4*by+3)
            lists.append(grp_sum(m))
    new16+=np.maximum.reduce(lists).sum(); ideal16+=sum(l.sum() for l in lists)/8
print('4x4 eighth-waves (max of 8 lists):',new16,'ratio',new16/cur,' ideal:',ideal16/cur)
# 8x2 blocks, eighth-waves
new82=0; ideal82=0
for hy in range(2):
    lists=[]
    for by in range(4):
        for bx in range(2):
            m=touches(x0+8*bx,x0+8*bx+7,y0+8*hy+2*by,y0+8*hy+2*by+1)
            lists.append(grp_sum(m))
    new82+=np.maximum.reduce(lists).sum(); ideal82+=sum(l.sum() for l in lists)/8
print('8x2 eighth-waves (max of 8 lists):',new82,'ratio',new82/cur,' ideal:',ideal82/cur)
# --- G = 8 (GS3D_BLEND_GROUPS=8) beside G = 4: wave-steps against the staging batch, and what a quadrant pre-test would see ---
def grp(mask,g):
    u,inv=np.unique(g,return_inverse=True); return np.bincount(inv,weights=mask,minlength=len(u))
for name,bw,bh,nx,ny in (('8x4 (G=4)',8,4,2,2),('4x4 (G=8)',4,4,4,2)):
    masks={}
    for hy in range(2):
        for by in range(ny):
            for bx in range(nx):
                masks[(hy,by,bx)]=touches(x0+bw*bx,x0+bw*bx+bw-1,y0+8*hy+bh*by,y0+8*hy+bh*by+bh-1)
    tot=sum(m.sum() for m in masks.values())
    print(name,'block entries',tot,'per pair',tot/D,' ideal wave-steps (entries / lists per wave)',tot/(nx*ny))
    for B in (128,256,512,10**9):
        gb=tile*100000+pos//B
        s=0
        for hy in range(2):
            s+=np.maximum.reduce([grp(masks[(hy,by,bx)],gb) for by in range(ny) for bx in range(nx)]).sum()
        print('  batch',B if B<10**9 else 'whole tile','wave-steps (max of the lists)',s,' / ideal',s/(tot/(nx*ny)))
# quadrant pre-test (8x8): pass rate per pair, and how often a staging wave (64 consecutive pairs of a tile) has an EMPTY quadrant ballot
wv=tile*100000+pos//64
for qy in range(2):
    for qx in range(2):
        m=q[(qy,qx)]; per_wave=grp(m,wv)
        print('quadrant',(qy,qx),'pass rate %.3f'%m.mean(),' staging waves with an empty ballot %.3f'%(per_wave==0).mean())
if ARGS.drop_finished:
    e,s=staging_g8(ARGS.slack,True)
    print('4x4 (G=8), batch 128, slack %g, finished blocks left off: block entries %d wave-steps %d'%(ARGS.slack,e,s))
